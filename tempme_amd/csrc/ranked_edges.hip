// Ranked explanation edges on gfx950: the distinct edges behind a prediction, best first.
//
// retrieve_explanation gives one weight per subgraph SLOT ([3B, N] hop-1 and [3B, N^2] hop-2 rows); the same edge
// id sits in several slots of a row and again in the other side's row of the same (src, tgt) pair.  A group is one
// or two rows; its entries are the rows' slots in group_rows order (entry p * ne + s: position p in the group, slot s,
// hop-1 slots first, ne = n or n + n^2); an entry is live iff its node record is nonzero and its edge id positive.
// Per group this kernel gives every distinct live edge id once, with
//     score = the maximum over the edge's live entries (fp32 comparison, -0 == +0, a NaN loses to every number),
//     slot  = the edge's lowest live entry index,   mult = the number of its live entries,
// ordered by score descending (NaN last), equal scores by edge id ascending, the first k of them stored and the
// rest of the k positions padded (eid 0, score 0, slot -1, mult 0); count = all distinct live edges (may exceed k).
// Comparisons only, no floating-point arithmetic: a score goes through an order-preserving u32 key and back, so the
// stored bits are an entry's own, except that a zero maximum is stored as +0.0 and an all-NaN one as 0x7FC00000.
//
// One workgroup per group, everything in LDS (12 bytes per entry of the padded power-of-two capacity P):
//   1. stage   key (eid << 32 | entry) or all ones for a dead entry, and the score key by entry
//   2. sort    bitonic, ascending: an edge's entries become one run, lowest entry first, dead entries last
//   3. scan    the score key follows its entry; a segmented Hillis-Steele scan leaves the run's maximum and length
//              in its last element (the low key word carries entry | length << 13 | run-start flag << 31)
//   4. compact run tails ranked by wave ballots and one pass over the waves' totals: distinct edge j gets the key
//              (~score key << 32 | eid) and the payload slot | mult << 13
//   5. sort    bitonic over the next power of two >= count, ascending = score descending, then eid ascending
//   6. store   the first k
// Keys of live entries are unique in both sorts and no atomic is used, so every launch gives the same bits.  A thread
// owns the elements tid + e * T in the scan and the compaction: consecutive lanes, consecutive 8-byte keys, no bank
// conflict there or in the sort steps with partner distance >= 32; the closer steps split a 32-lane group over two
// 256-byte rows of banks (2-way).  The steps are bound by LDS latency, not bandwidth: see the launch table below.
#include "common.h"

namespace tmk {

constexpr int kReMaxEntries = 8192;
constexpr uint32_t kReDead = 0xFFFFFFFFu;      // high key word of a dead entry
constexpr uint32_t kReIdxBits = 13, kReIdxMask = (1u << kReIdxBits) - 1u;
constexpr uint32_t kReCntField = 0x3FFFu << kReIdxBits, kReHead = 0x80000000u;

struct ReArgs {
    const float *imp1, *imp2;
    const int32_t *node1, *node2, *eid1, *eid2;
    const int32_t *group_rows;
    int32_t rows, n, hops, R, k, np;           // np: the power of two >= R * ne that sort 1 covers
    int32_t *out_eid;
    float *out_score;
    int32_t *out_slot, *out_mult, *out_count, *err;
};

// fp32 -> u32, order-preserving: a < b  <=>  key(a) < key(b); -0 and +0 share a key; every NaN gets 0, below -inf
__device__ __forceinline__ uint32_t re_score_key(float f) {
    if (f != f) return 0u;
    uint32_t b = __float_as_uint(f);
    if (f == 0.0f) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float re_key_score(uint32_t k) {
    if (k == 0u) return __uint_as_float(0x7FC00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

__device__ __forceinline__ uint64_t re_u64(uint2 v) { return ((uint64_t)v.y << 32) | v.x; }

// compare-exchange t of the step with partner distance j in the stage of run length k2
template <bool PAY>
__device__ __forceinline__ void re_exchange(uint2 *K, uint32_t *V, int t, int j, int k2) {
    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
    const uint2 a = K[i], b = K[l];
    const uint64_t ka = re_u64(a), kb = re_u64(b);
    if (ka != kb && (ka > kb) == ((i & k2) == 0)) {
        K[i] = b;
        K[l] = a;
        if (PAY) {
            const uint32_t x = V[i];
            V[i] = V[l];
            V[l] = x;
        }
    }
}

// LDS accesses of one wave stay in program order for the compiler (the hardware serves a wave's LDS instructions
// in the order it issued them): enough between two steps whose keys no other wave touches
__device__ __forceinline__ void re_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ascending bitonic sort of K[0, n) (n a power of two, the same in every thread), V following K when PAY.  A wave's
// 64 consecutive exchanges t cover the 128 keys [2 t0, 2 t0 + 128) in every step with partner distance <= 32, so
// those steps of a stage need no workgroup barrier between them: 20 barriers instead of 55 at n = 1024.
template <int T, bool PAY>
__device__ __forceinline__ void re_bitonic(uint2 *K, uint32_t *V, int n, int tid) {
    for (int k2 = 2; k2 <= n; k2 <<= 1) {
        int j = k2 >> 1;
        for (; j > 32; j >>= 1) {
            for (int t = tid; t < (n >> 1); t += T) re_exchange<PAY>(K, V, t, j, k2);
            __syncthreads();
        }
        for (int t = tid; t < (n >> 1); t += T)
            for (int jj = j; jj > 0; jj >>= 1) {
                re_exchange<PAY>(K, V, t, jj, k2);
                re_wave_sync();
            }
        __syncthreads();
    }
}

template <int P, int T>
__global__ void __launch_bounds__(T) ranked_edges_kernel(ReArgs a) {
    extern __shared__ uint2 re_lds[];
    constexpr int E = P / T, NW = T / 64;
    uint2 *K = re_lds;                                        // [P] {low, high} key words
    uint32_t *V = reinterpret_cast<uint32_t *>(K + P);        // [P] score keys, then sort 2's payload
    uint32_t *S = V + P;                                      // [2][E * NW] tails per (round, wave), their prefix
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n, nn = a.hops == 2 ? n * n : 0, ne = n + nn, total = a.R * ne;

    // ---- 1. stage
    for (int p = 0; p < a.R; ++p) {
        const int32_t row = a.group_rows[(int64_t)blockIdx.x * a.R + p];
        const bool ok = row >= 0 && row < a.rows;
        if (!ok && row != -1 && tid == 0 && a.err) *a.err = TM_E_ARG;
        for (int s = tid; s < ne; s += T) {
            uint2 key = make_uint2(kReDead, kReDead);
            uint32_t sk = 0u;
            if (ok) {
                int32_t nd, e;
                float f;
                if (s < n) {
                    const int64_t o = (int64_t)row * n + s;
                    nd = a.node1[o], e = a.eid1[o], f = a.imp1[o];
                } else {
                    const int64_t o = (int64_t)row * nn + (s - n);
                    nd = a.node2[o], e = a.eid2[o], f = a.imp2[o];
                }
                if (nd != 0 && e > 0) {
                    key = make_uint2((uint32_t)(p * ne + s), (uint32_t)e);
                    sk = re_score_key(f);
                }
            }
            K[p * ne + s] = key;
            V[p * ne + s] = sk;
        }
    }
    for (int t = total + tid; t < P; t += T) {
        K[t] = make_uint2(kReDead, kReDead);
        V[t] = 0u;
    }
    __syncthreads();

    // ---- 2. runs of equal edge id, lowest entry first
    re_bitonic<T, false>(K, V, a.np, tid);

    // ---- 3. the score key follows its entry; run-start flags; segmented scan of (max score key, length)
    uint32_t lo[E], v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = e * T + tid;
        const uint2 k = K[i];
        const bool live = k.y != kReDead;
        const bool head = !live || i == 0 || K[i - 1].y != k.y;
        v[e] = live ? V[k.x] : 0u;
        lo[e] = (k.x & kReIdxMask) | (1u << kReIdxBits) | (head ? kReHead : 0u);
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = e * T + tid;
        V[i] = v[e];
        K[i].x = lo[e];
    }
    __syncthreads();
    for (int d = 1; d < a.np; d <<= 1) {
        uint32_t plo[E], pv[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = e * T + tid;
            const bool take = !(lo[e] & kReHead) && i >= d;
            plo[e] = take ? K[i - d].x : 0u;
            pv[e] = take ? V[i - d] : 0u;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = e * T + tid;
            if (!(lo[e] & kReHead) && i >= d) {
                v[e] = max(v[e], pv[e]);
                lo[e] = (lo[e] + (plo[e] & kReCntField)) | (plo[e] & kReHead);
                V[i] = v[e];
                K[i].x = lo[e];
            }
        }
        __syncthreads();
    }

    // ---- 4. run tails -> distinct edges, in edge-id order
    uint2 key2[E];
    uint32_t pay2[E];
    int wpre[E];                                              // tails before this lane in its wave, -1: no tail
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = e * T + tid;
        const uint32_t eid = K[i].y;
        const bool tail = eid != kReDead && (i == P - 1 || K[i + 1].y != eid);
        const unsigned long long m = __ballot(tail);
        wpre[e] = tail ? __popcll(m & ((1ull << lane) - 1ull)) : -1;
        if (lane == 0) S[e * NW + wave] = (uint32_t)__popcll(m);
        key2[e] = make_uint2(eid, ~v[e]);
        pay2[e] = 0u;
        if (tail) {
            const uint32_t mult = (lo[e] & kReCntField) >> kReIdxBits;
            const uint32_t slot = K[i - (int)mult + 1].x & kReIdxMask;
            pay2[e] = slot | (mult << kReIdxBits);
        }
    }
    __syncthreads();                                          // S complete; every read of the sorted image done
    if (tid < E * NW) {                                       // exclusive prefix of the E * NW <= 128 totals
        uint32_t acc = 0u;
#pragma unroll 1
        for (int q = 0; q < tid; ++q) acc += S[q];
        S[E * NW + tid] = acc;
    }
    __syncthreads();
    const int count = (int)(S[2 * E * NW - 1] + S[E * NW - 1]);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (wpre[e] >= 0) {
            const int j = (int)S[E * NW + e * NW + wave] + wpre[e];
            K[j] = key2[e];
            V[j] = pay2[e];
        }
    }
    for (int t = count + tid; t < P; t += T) {
        K[t] = make_uint2(kReDead, kReDead);
        V[t] = 0u;
    }
    __syncthreads();

    // ---- 5. score descending, then edge id ascending
    int n2 = 1;
    while (n2 < count) n2 <<= 1;
    re_bitonic<T, true>(K, V, n2, tid);

    // ---- 6. store
    const int64_t ob = (int64_t)blockIdx.x * a.k;
    for (int j = tid; j < a.k; j += T) {
        int32_t oe = 0, os = -1, om = 0;
        float of = 0.0f;
        if (j < count) {
            const uint2 k = K[j];
            const uint32_t pz = V[j];
            oe = (int32_t)k.x;
            of = re_key_score(~k.y);
            os = (int32_t)(pz & kReIdxMask);
            om = (int32_t)(pz >> kReIdxBits);
        }
        a.out_eid[ob + j] = oe;
        a.out_score[ob + j] = of;
        a.out_slot[ob + j] = os;
        a.out_mult[ob + j] = om;
    }
    if (tid == 0) a.out_count[blockIdx.x] = count;
}

template <int P, int T>
static int re_launch(const ReArgs &a, int32_t n_groups, hipStream_t s) {
    const size_t lds = (size_t)P * 12 + (size_t)2 * (P / T) * (T / 64) * 4;
    TM_HIP(hipFuncSetAttribute((const void *)ranked_edges_kernel<P, T>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
    ranked_edges_kernel<P, T><<<dim3((unsigned)n_groups), T, lds, s>>>(a);
    return TM_OK;
}

}  // namespace tmk

using namespace tmk;

extern "C" int tm_ranked_edges(const float *imp1, const float *imp2, const int32_t *node1, const int32_t *node2,
                               const int32_t *eid1, const int32_t *eid2, int32_t rows, int32_t n, int32_t hops,
                               const int32_t *group_rows, int32_t n_groups, int32_t rows_per_group, int32_t k,
                               int32_t *out_eid, float *out_score, int32_t *out_slot, int32_t *out_mult,
                               int32_t *out_count, int32_t *err_flag, void *stream) {
    if (rows < 0 || n < 1 || n_groups < 0 || (hops != 1 && hops != 2) || (rows_per_group != 1 && rows_per_group != 2))
        return fail(TM_E_ARG, "tm_ranked_edges: rows >= 0, n >= 1, n_groups >= 0, hops 1 or 2 and 1 or 2 rows per "
                              "group are required");
    const int64_t ne = hops == 2 ? (int64_t)n + (int64_t)n * n : n, total = ne * rows_per_group;
    if (total > kReMaxEntries)
        return fail(TM_E_UNSUPPORTED, "tm_ranked_edges: " + std::to_string(total) + " entries per group (" +
                                          std::to_string(rows_per_group) + " rows of " + std::to_string(ne) +
                                          ") exceed the limit of " + std::to_string(kReMaxEntries));
    if (k < 1 || k > total)
        return fail(TM_E_ARG, "tm_ranked_edges: k = " + std::to_string(k) + " is outside [1, " +
                                  std::to_string(total) + "], the entries of a group");
    if (n_groups == 0) return TM_OK;
    if (!imp1 || !node1 || !eid1 || (hops == 2 && (!imp2 || !node2 || !eid2)) || !group_rows || !out_eid ||
        !out_score || !out_slot || !out_mult || !out_count)
        return fail(TM_E_ARG, "tm_ranked_edges: NULL pointer");
    int32_t np = 1;
    while (np < total) np <<= 1;
    const ReArgs a{imp1, imp2, node1, node2, eid1, eid2, group_rows, rows, n, hops, rows_per_group, k, np,
                   out_eid, out_score, out_slot, out_mult, out_count, err_flag};
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t pe = prof_begin(s);
    // the padded capacity per launch: N = 20 with two rows (840 entries) sorts 1024 keys, not 8192.  One thread per
    // exchange of a sort step up to 1024 threads: the steps are LDS-latency bound, and at 1024 keys 512 threads
    // measured 0.033 ms per 200 groups against 0.047 with 256 and 0.031 with 1024 (which is slower at 1,024 groups,
    // 0.073 against 0.057 ms: fewer workgroups fit a CU)
    int rc;
    if (total <= 1024) rc = re_launch<1024, 512>(a, n_groups, s);
    else if (total <= 2048) rc = re_launch<2048, 1024>(a, n_groups, s);
    else if (total <= 4096) rc = re_launch<4096, 1024>(a, n_groups, s);
    else rc = re_launch<8192, 1024>(a, n_groups, s);
    if (rc != TM_OK) return rc;
    TM_CHECK_LAUNCH();
    prof_end("ranked_edges_kernel", s, pe);
    return TM_OK;
}
