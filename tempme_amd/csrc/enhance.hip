// Motif-enhanced link prediction (models/explainer_new.py:203-306) on gfx950: the walk-importance weights of
// compute_walk_importance (:260-306) and the per-event tail of the pooled encoder (tm_encoder_pool_fwd,
// encoder.hip), whose walk kernels end at attention.MLP's hidden layer.
//
// Kernels:
//   walk_importance_kernel  one workgroup per group (one reference call): recency and degree weights of the
//                           group's B*W walks, their three group statistics in fp64, and the per-event
//                           normalisation; fixed reduction orders, so the weights are bitwise reproducible
//   pool_tail_kernel        one workgroup per (group, event): the event's partial rows summed in order, attention.MLP's
//                           last Linear applied once to the sum, and the event's category histogram
#include "encoder_common.h"

namespace tmk {

constexpr int WI_TPB = 1024;

// sum over the workgroup in a fixed order (wave butterflies, then the waves' partials in order)
__device__ __forceinline__ double wi_block_sum(double v, double *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int k = 0; k < nw; ++k) s += red[k];
    return s;
}

// |cut - max_p ts| (:279-281) and the mean degree of the walk's valid (> 0) node entries (:289-295) of walk w of
// event b; a node id outside the table sets *err_flag and counts as padding
__device__ __forceinline__ void wi_walk(const float *__restrict__ degree, int32_t n_nodes, const int32_t *__restrict__ n6,
                                        const float *__restrict__ t3, float cut, int32_t *__restrict__ err_flag,
                                        float &diff, float &avg) {
    diff = fabsf(cut - fmaxf(fmaxf(t3[0], t3[1]), t3[2]));
    float sum = 0.f, cnt = 0.f;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int32_t n = n6[k];
        if (n < 0 || n >= n_nodes) {
            if (err_flag) *err_flag = TM_E_ARG;
        } else if (n > 0) {
            sum += degree[n];
            cnt += 1.f;
        }
    }
    avg = sum / (cnt + 1e-6f);
}

__global__ void __launch_bounds__(WI_TPB) walk_importance_kernel(const float *__restrict__ degree, int32_t n_nodes,
                                                                 int32_t B, int32_t W, const int32_t *__restrict__ node6,
                                                                 const float *__restrict__ ts3,
                                                                 const double *__restrict__ cut, float *__restrict__ out,
                                                                 int32_t *__restrict__ err_flag) {
    __shared__ double red[WI_TPB / 64];
    const int64_t g = blockIdx.x;
    const int32_t nw = B * W;
    const int32_t *n6 = node6 + g * (int64_t)nw * 6;
    const float *t3 = ts3 + g * (int64_t)nw * 3;
    const double *cg = cut + g * B;
    float *og = out + g * (int64_t)nw;
    // the group's means (fp64 sums of the fp32 elements, thread-strided, then wi_block_sum)
    double sd = 0.0, sa = 0.0;
    for (int32_t w = threadIdx.x; w < nw; w += WI_TPB) {
        float diff, avg;
        wi_walk(degree, n_nodes, n6 + (int64_t)w * 6, t3 + (int64_t)w * 3, (float)cg[w / W], nullptr, diff, avg);
        sd += (double)diff;
        sa += (double)avg;
    }
    const double md = wi_block_sum(sd, red) / (double)nw, ma = wi_block_sum(sa, red) / (double)nw;
    double vd = 0.0, va = 0.0;
    for (int32_t w = threadIdx.x; w < nw; w += WI_TPB) {
        float diff, avg;
        wi_walk(degree, n_nodes, n6 + (int64_t)w * 6, t3 + (int64_t)w * 3, (float)cg[w / W], nullptr, diff, avg);
        const double dd = (double)diff - md, da = (double)avg - ma;
        vd += dd * dd;
        va += da * da;
    }
    // unbiased std (torch.std of one element is NaN) and the mean, rounded to fp32 as torch returns them
    const double qd = wi_block_sum(vd, red), qa = wi_block_sum(va, red);
    const float nanf_ = __builtin_nanf("");
    const float std_d = nw > 1 ? (float)sqrt(qd / (double)(nw - 1)) : nanf_;
    const float std_a = nw > 1 ? (float)sqrt(qa / (double)(nw - 1)) : nanf_;
    const float mean_a = (float)ma;
    // walk_importance = 0.5 recency + 0.5 degree weight (:285, :298, :301), kept in `out` for the normalisation
    for (int32_t w = threadIdx.x; w < nw; w += WI_TPB) {
        float diff, avg;
        wi_walk(degree, n_nodes, n6 + (int64_t)w * 6, t3 + (int64_t)w * 3, (float)cg[w / W], err_flag, diff, avg);
        const float rec = expf(-diff / (std_d + 1e-6f));
        const float z = (avg - mean_a) / (std_a + 1e-6f);
        const float dw = 1.f / (1.f + expf(-z));
        og[w] = 0.5f * rec + 0.5f * dw;
    }
    __syncthreads();
    // per event: imp / (sum_w imp / W + 1e-6) (:304); 16 lanes per event, each summing walks l, l + 16, ... in
    // fp64, then a butterfly over the 16 (fixed order)
    const int sub = threadIdx.x & 15;
    for (int32_t b = threadIdx.x >> 4; b < B; b += WI_TPB / 16) {
        float *row = og + (int64_t)b * W;
        double s = 0.0;
        for (int32_t w = sub; w < W; w += 16) s += (double)row[w];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);
        const float den = (float)s / (float)W + 1e-6f;
        for (int32_t w = sub; w < W; w += 16) row[w] = row[w] / den;
    }
}

constexpr int TAIL_TPB = 256;

__global__ void __launch_bounds__(TAIL_TPB) pool_tail_kernel(Lin a2, int32_t W, int32_t n_part, int32_t h, int32_t do_cat,
                                                             const float *__restrict__ part,
                                                             const float *__restrict__ wgt,
                                                             const int32_t *__restrict__ cat, float *__restrict__ out,
                                                             int64_t ld_out) {
    __shared__ float s_x[256];      // the pooled hidden vector (h <= 256)
    __shared__ float s_p[TAIL_TPB];
    __shared__ float s_sw;
    const int64_t e = blockIdx.x;
    const int i = threadIdx.x;
    // the event's partial rows in nrep = 256 / h contiguous chunks, one per thread of a column, then the chunks'
    // sums in order (fixed for a shape, so the result is reproducible)
    const int nrep = TAIL_TPB / h, rep = i / h, c = i - rep * h;
    if (rep < nrep) {
        const int32_t k0 = (int32_t)((int64_t)rep * n_part / nrep), k1 = (int32_t)((int64_t)(rep + 1) * n_part / nrep);
        const float *p = part + e * n_part * (int64_t)h + c;
        float s = 0.f;
        for (int32_t k = k0; k < k1; ++k) s += p[(int64_t)k * h];
        s_p[i] = s;
    }
    if (i == TAIL_TPB - 1) {
        float s = 0.f;
        for (int32_t w = 0; w < W; ++w) s += wgt[e * W + w];
        s_sw = s;
    }
    __syncthreads();
    if (i < h) {
        float s = 0.f;
        for (int r = 0; r < nrep; ++r) s += s_p[r * h + i];
        s_x[i] = s;
    }
    __syncthreads();
    float *o = out + e * ld_out;
    if (i < h) {
        // row i of a2 from the fragment pack: element (o, c) at ((t nq + q) 64 + l) 4 + s, o = 16 t + (l & 15),
        // c = 16 q + 4 (l >> 4) + s
        const float4 *wrow = a2.w + (int64_t)(i >> 4) * a2.nq * 64 + (i & 15);
        float acc = a2.b[i] * s_sw;
        for (int q = 0; 16 * q < h; ++q) {
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const float4 wv = wrow[q * 64 + gq * 16];
                const float *x = s_x + 16 * q + 4 * gq;
                acc = __builtin_fmaf(wv.x, x[0], acc);
                acc = __builtin_fmaf(wv.y, x[1], acc);
                acc = __builtin_fmaf(wv.z, x[2], acc);
                acc = __builtin_fmaf(wv.w, x[3], acc);
            }
        }
        o[i] = acc;
    }
    if (do_cat && i < 12) {   // compute_catogory_feautres(level="node") (:308-313): the unweighted histogram
        int32_t n = 0;
        for (int32_t w = 0; w < W; ++w) n += cat[e * W + w] == i;
        o[h + i] = (float)n;
    }
}

void launch_pool_tail(const Lin &a2, int64_t n_events, int32_t W, int32_t n_part, int32_t h, int32_t do_cat,
                      const float *part, const float *wgt, const int32_t *cat, float *out, int64_t ld_out,
                      hipStream_t s) {
    pool_tail_kernel<<<dim3((unsigned)n_events), TAIL_TPB, 0, s>>>(a2, W, n_part, h, do_cat, part, wgt, cat, out, ld_out);
}

}  // namespace tmk

using namespace tmk;

extern "C" int tm_walk_importance(const float *node_degree, int32_t n_nodes, int32_t n_groups, int32_t B, int32_t W,
                                  const int32_t *node6, const float *ts3, const double *cut, float *out_wgt,
                                  int32_t *err_flag, void *stream) {
    if (n_groups < 0 || B < 0 || W < 0 || n_nodes <= 0) return fail(TM_E_ARG, "tm_walk_importance: bad arguments");
    if ((int64_t)B * W > INT32_MAX) return fail(TM_E_UNSUPPORTED, "tm_walk_importance: B * W above 2^31 - 1");
    if ((int64_t)n_groups * B * W == 0) return TM_OK;
    if (!node_degree || !node6 || !ts3 || !cut || !out_wgt) return fail(TM_E_ARG, "tm_walk_importance: NULL pointer");
    hipStream_t s = S_(stream);
    hipEvent_t pe = prof_begin(s);
    walk_importance_kernel<<<dim3((unsigned)n_groups), WI_TPB, 0, s>>>(node_degree, n_nodes, B, W, node6, ts3, cut, out_wgt,
                                                                       err_flag);
    TM_CHECK_LAUNCH();
    prof_end("walk_importance_kernel", s, pe);
    return TM_OK;
}
