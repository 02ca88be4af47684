// Per-batch evaluation metrics on gfx950: average precision and ROC-AUC of a score vector against binary
// labels (sklearn.metrics.average_precision_score / roc_auc_score, which temp_exp_main.py:463-478, :253-263,
// :633-649 and learn_base.py:43-73 call on the host for every batch).
//
// Both figures are rank statistics, written here with counts so that ties need no sort order.  A label is
// positive iff it is > 0.5; P positives, Nn = n - P negatives; for element i
//
//     ge_i  = #{j : s_j >= s_i}      pge_i = #{j positive : s_j >= s_i}      pgt_i = #{j positive : s_j > s_i}
//
//     AP  = (1 / P) sum_{i positive} pge_i / ge_i                   P = 0           -> 0.0
//     AUC = sum_{i negative} (pgt_i + pge_i) / (2 P Nn)             P = 0 or Nn = 0 -> NaN
//
// (precision at the threshold s_i is pge_i / ge_i, and every positive adds 1 / P of recall there; a
// negative counts the positives above it once and the positives tied with it half).  Scores are compared as
// the fp32 values given (-0.0 == 0.0).  A NaN score makes both figures of its vector NaN.
//
// One workgroup of 256 threads per vector.  The scores are staged into LDS twice: a[j] = s_j and
// p[j] = s_j for a positive, NaN otherwise (a NaN compares false, so p counts positives only), both padded
// with NaN to a multiple of four.  Each thread owns EPT elements at a time in registers and streams all of a
// and p from LDS as 16-byte same-address reads (broadcast), three compare-and-count per pair.  The counts
// are integers; AUC's numerator (below 2^27 at n = 8192) is summed in integers and divided once in fp64;
// AP's terms are summed in fp64 per thread in element order, then by a fixed tree through LDS: no float
// atomics, the same bits from every launch.
#include <cmath>

#include "common.h"

namespace tmk {

constexpr int kRankThreads = 256;
constexpr int kRankMaxN = 8192;

template <int EPT>
__global__ void __launch_bounds__(kRankThreads)
    rank_metrics_kernel(const float *__restrict__ score, int64_t score_stride, const float *__restrict__ label,
                        int64_t label_stride, int32_t n, double *__restrict__ out) {
    extern __shared__ float4 lds4[];
    const int tid = threadIdx.x;
    const int npad = (n + 3) & ~3;
    float *a = reinterpret_cast<float *>(lds4), *p = a + npad;
    const float *s = score + (int64_t)blockIdx.x * score_stride;
    const float *l = label + (int64_t)blockIdx.x * label_stride;
    const float qnan = __builtin_nanf("");
    uint32_t n_pos = 0, has_nan = 0;
    for (int j = tid; j < npad; j += kRankThreads) {
        float sj = qnan, pj = qnan;
        if (j < n) {
            sj = s[j];
            const bool pos = l[j] > 0.5f;
            pj = pos ? sj : qnan;
            n_pos += pos;
            has_nan |= (sj != sj);
        }
        a[j] = sj;
        p[j] = pj;
    }
    __syncthreads();

    double ap_sum = 0.0;
    uint32_t auc_num = 0;
    const float4 *a4 = lds4, *p4 = lds4 + (npad >> 2);
    for (int base = 0; base < n; base += kRankThreads * EPT) {
        float si[EPT];
        uint32_t ge[EPT], pge[EPT], pgt[EPT];
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int i = base + e * kRankThreads + tid;
            si[e] = i < n ? a[i] : qnan;      // an element past n counts nothing and is skipped below
            ge[e] = pge[e] = pgt[e] = 0;
        }
        for (int j4 = 0; j4 < (npad >> 2); ++j4) {
            const float4 av = a4[j4], pv = p4[j4];
            const float as[4] = {av.x, av.y, av.z, av.w}, ps[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
#pragma unroll
                for (int e = 0; e < EPT; ++e) {
                    ge[e] += as[c] >= si[e];
                    pge[e] += ps[c] >= si[e];
                    pgt[e] += ps[c] > si[e];
                }
            }
        }
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int i = base + e * kRankThreads + tid;
            if (i < n) {
                const float pi = p[i];
                if (pi == pi) ap_sum += (double)pge[e] / (double)ge[e];     // ge >= 1: the element itself
                else auc_num += pgt[e] + pge[e];
            }
        }
    }
    __syncthreads();      // every read of a and p is done: the region becomes the reduction's

    double *r_ap = reinterpret_cast<double *>(lds4);
    uint32_t *r_num = reinterpret_cast<uint32_t *>(r_ap + kRankThreads);
    uint32_t *r_pos = r_num + kRankThreads, *r_nan = r_pos + kRankThreads;
    r_ap[tid] = ap_sum;
    r_num[tid] = auc_num;
    r_pos[tid] = n_pos;
    r_nan[tid] = has_nan;
    __syncthreads();
    for (int w = kRankThreads / 2; w > 0; w >>= 1) {
        if (tid < w) {
            r_ap[tid] += r_ap[tid + w];
            r_num[tid] += r_num[tid + w];
            r_pos[tid] += r_pos[tid + w];
            r_nan[tid] |= r_nan[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double P = (double)r_pos[0], Nn = (double)n - P;
        const double dnan = __builtin_nan("");
        double ap = P > 0.0 ? r_ap[0] / P : 0.0;
        double auc = (P > 0.0 && Nn > 0.0) ? (double)r_num[0] / (2.0 * P * Nn) : dnan;
        if (r_nan[0]) ap = auc = dnan;
        double *o = out + (int64_t)blockIdx.x * 2;
        o[0] = ap;
        o[1] = auc;
    }
}

// bytes of dynamic LDS: the two staged arrays, or the reduction's four arrays where those are smaller
static size_t rank_lds_bytes(int32_t n) {
    const size_t stage = (size_t)2 * ((n + 3) & ~3) * sizeof(float);
    const size_t reduce = (size_t)kRankThreads * (sizeof(double) + 3 * sizeof(uint32_t));
    return stage > reduce ? stage : reduce;
}

}  // namespace tmk

using namespace tmk;

extern "C" int tm_rank_metrics(const float *score, int64_t score_stride, const float *label, int64_t label_stride,
                               int32_t n_vec, int32_t n, double *out, void *stream) {
    if (n <= 0 || n_vec < 0) return fail(TM_E_ARG, "tm_rank_metrics: n must be positive and n_vec non-negative");
    if (n > kRankMaxN)
        return fail(TM_E_UNSUPPORTED, "tm_rank_metrics: n = " + std::to_string(n) + " exceeds the limit of " +
                                          std::to_string(kRankMaxN) + " scores per vector");
    if (score_stride < n || (label_stride != 0 && label_stride < n))
        return fail(TM_E_ARG, "tm_rank_metrics: a row stride is below n");
    if (n_vec == 0) return TM_OK;
    if (!score || !label || !out) return fail(TM_E_ARG, "tm_rank_metrics: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t pe = prof_begin(s);
    const size_t lds = rank_lds_bytes(n);
    // one pass over the elements for n <= 256; four elements per thread and pass beyond
    if (n <= kRankThreads)
        rank_metrics_kernel<1><<<dim3((unsigned)n_vec), kRankThreads, lds, s>>>(score, score_stride, label,
                                                                                 label_stride, n, out);
    else
        rank_metrics_kernel<4><<<dim3((unsigned)n_vec), kRankThreads, lds, s>>>(score, score_stride, label,
                                                                                 label_stride, n, out);
    TM_CHECK_LAUNCH();
    prof_end("rank_metrics_kernel", s, pe);
    return TM_OK;
}
