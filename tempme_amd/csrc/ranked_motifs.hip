// Ranked motif instances on gfx950: the distinct temporal motifs (walks of three events) behind a prediction, best
// first, their category profile, and the subgraph mask of the top m of them.
//
// The encoder scores every sampled walk (imp [rows, W]); walks are sampled with replacement, so one motif instance --
// one ordered triple of edge ids (e0, e1, e2) -- sits in several of a row's W walks and again in the partner row of
// the pair.  A group is one or two rows; its entries are the rows' walks in group_rows order (entry p * W + w); an
// entry is live iff eid3[row, w, 0] > 0 (the walk left its root) and its category is one of the 12.  Per group
// ranked_motifs_kernel gives every distinct live triple once (all 96 bits compared), with
//     score = the maximum over the instance's live entries (fp32 comparison, -0 == +0, a NaN loses to every number),
//     walk  = its lowest live entry index,  mult = the number of its live entries,  cat = the category of entry walk,
// ordered by score descending (NaN last), equal scores by the triple ascending (lexicographic, ids unsigned), the
// first k stored and the rest of the k positions padded (eids 0, score 0, walk -1, mult 0, cat -1); count = all
// distinct live instances.  Per group and category it also gives the live ENTRIES' number, maximum and fp64 sum.
//
// Algorithm: rank by counting, not the bitonic sort + segmented scan of ranked_edges.hip.  A group has at most 1024
// entries (the workload's N = 20, M = 3 gives 60 per row, 120 per pair) against ranked_edges' 8192, and a 96-bit
// triple plus its entry index does not fit the 64-bit sort key there.  One thread owns one entry:
//   1. stage   {e0, e1, e2, score key} (e0 = 0: dead), the category and the score's bits by entry, in LDS
//   2. group   every live thread walks all entries (all lanes read the same 16 bytes: an LDS broadcast, no bank
//              conflict) and takes the maximum score key, the number and the lowest index of the entries that carry
//              its triple; it is the instance's head iff that lowest index is its own
//   3. rank    heads publish {~score key, e0, e1, e2}, every other thread all ones; a head's rank is the number of
//              published keys below its own (heads' keys are distinct, so ranks are 0 .. count - 1, each once);
//              count comes from the waves' ballots
//   4. store   a head of rank < k writes its position; the threads together pad positions >= min(count, k)
//   5. profile thread c < 12 walks the entries once, in ascending order: one fp64 accumulator per category, so a plain
//              sequential loop on the host reproduces the sum bit for bit
// Two passes of `total` broadcast reads per thread and two workgroup barriers replace ~110 dependent exchange steps;
// at 120 entries that is 240 reads per thread.  Comparisons only (a score goes through ranked_edges' order-preserving
// u32 key and back), no atomics, no floating-point arithmetic except the fp64 sums: every launch gives the same bits.
//
// motif_mask_kernel: the node records a base model scores when only the events of a row's top m motifs are kept.
#include "common.h"

namespace tmk {

constexpr int kRmMaxEntries = 1024;
constexpr int kRmCats = 12;
constexpr int kRmMaxM = 64;                    // m values per tm_motif_mask call (they travel by value)
constexpr uint32_t kRmNone = 0xFFFFFFFFu;

struct RmArgs {
    const int32_t *eid3, *cat;
    const float *imp;
    const int32_t *group_rows;
    int32_t rows, W, R, k;
    int32_t *out_eid;
    float *out_score;
    int32_t *out_walk, *out_mult, *out_cat, *out_count, *cat_n;
    float *cat_max;
    double *cat_sum;
    int32_t *err;
};

// fp32 -> u32, order-preserving: a < b  <=>  key(a) < key(b); -0 and +0 share a key; every NaN gets 0, below -inf
// (the conventions of ranked_edges.hip)
__device__ __forceinline__ uint32_t rm_score_key(float f) {
    if (f != f) return 0u;
    uint32_t b = __float_as_uint(f);
    if (f == 0.0f) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float rm_key_score(uint32_t k) {
    if (k == 0u) return __uint_as_float(0x7FC00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// one thread per entry: blockDim.x = the entries of a group rounded up to whole waves
__global__ void __launch_bounds__(kRmMaxEntries) ranked_motifs_kernel(RmArgs a) {
    extern __shared__ uint4 rm_lds[];
    const int T = (int)blockDim.x, tid = threadIdx.x, total = a.R * a.W;
    uint4 *A = rm_lds;                                        // [T] {e0, e1, e2, score key}; e0 = 0: dead
    uint4 *H = A + T;                                         // [T] {~score key, e0, e1, e2} of a head, else all ones
    uint32_t *C = reinterpret_cast<uint32_t *>(H + T);        // [T] category, kRmNone for a dead entry
    uint32_t *F = C + T;                                      // [T] the score's bits
    uint32_t *S = F + T;                                      // [T / 64] heads per wave

    // ---- 1. stage
    uint4 me = make_uint4(0u, 0u, 0u, 0u);
    uint32_t my_cat = kRmNone, my_bits = 0u;
    if (tid < total) {
        const int p = tid / a.W, w = tid - p * a.W;
        const int32_t row = a.group_rows[(int64_t)blockIdx.x * a.R + p];
        const bool ok = row >= 0 && row < a.rows;
        if (!ok && row != -1 && w == 0 && a.err) *a.err = TM_E_ARG;
        if (ok) {
            const int64_t o = (int64_t)row * a.W + w;
            const int32_t c = a.cat[o];
            const float f = a.imp[o];
            if (c < 0 || c >= kRmCats) {
                if (a.err) *a.err = TM_E_ARG;
            } else if (a.eid3[3 * o] > 0) {
                me = make_uint4((uint32_t)a.eid3[3 * o], (uint32_t)a.eid3[3 * o + 1], (uint32_t)a.eid3[3 * o + 2],
                                rm_score_key(f));
                my_cat = (uint32_t)c;
                my_bits = __float_as_uint(f);
            }
        }
    }
    A[tid] = me;
    C[tid] = my_cat;
    F[tid] = my_bits;
    __syncthreads();

    // ---- 2. the entries that carry this thread's triple: maximum, number, lowest index
    const bool live = me.x != 0u;
    uint32_t best = 0u;
    int mult = 0, first = total;
    if (live) {
        for (int j = 0; j < total; ++j) {
            const uint4 b = A[j];
            if (b.x == me.x && b.y == me.y && b.z == me.z) {
                best = max(best, b.w);
                mult += 1;
                first = min(first, j);
            }
        }
    }
    const bool head = live && first == tid;

    // ---- 3. rank among the heads: score descending (NaN: key 0, so ~key last), then the triple ascending
    const uint4 mine = head ? make_uint4(~best, me.x, me.y, me.z) : make_uint4(kRmNone, kRmNone, kRmNone, kRmNone);
    H[tid] = mine;
    const unsigned long long hm = __ballot(head);
    if ((tid & 63) == 0) S[tid >> 6] = (uint32_t)__popcll(hm);
    __syncthreads();
    int count = 0;
    for (int q = 0; q < (T >> 6); ++q) count += (int)S[q];
    if (head) {
        const uint64_t hi = ((uint64_t)mine.x << 32) | mine.y, lo = ((uint64_t)mine.z << 32) | mine.w;
        int rank = 0;
        for (int j = 0; j < total; ++j) {
            const uint4 b = H[j];
            const uint64_t bhi = ((uint64_t)b.x << 32) | b.y, blo = ((uint64_t)b.z << 32) | b.w;
            rank += (bhi < hi || (bhi == hi && blo < lo)) ? 1 : 0;
        }
        // ---- 4. store
        if (rank < a.k) {
            const int64_t o = (int64_t)blockIdx.x * a.k + rank;
            a.out_eid[3 * o] = (int32_t)me.x;
            a.out_eid[3 * o + 1] = (int32_t)me.y;
            a.out_eid[3 * o + 2] = (int32_t)me.z;
            a.out_score[o] = rm_key_score(best);
            a.out_walk[o] = tid;
            a.out_mult[o] = mult;
            a.out_cat[o] = (int32_t)my_cat;
        }
    }
    for (int j = min(count, a.k) + tid; j < a.k; j += T) {
        const int64_t o = (int64_t)blockIdx.x * a.k + j;
        a.out_eid[3 * o] = a.out_eid[3 * o + 1] = a.out_eid[3 * o + 2] = 0;
        a.out_score[o] = 0.0f;
        a.out_walk[o] = -1;
        a.out_mult[o] = 0;
        a.out_cat[o] = -1;
    }
    if (tid == 0) a.out_count[blockIdx.x] = count;

    // ---- 5. category profile over the live entries, ascending entry order, one accumulator per category
    if (tid < kRmCats) {
        int n = 0;
        uint32_t mk = 0u;
        double sum = 0.0;
        for (int j = 0; j < total; ++j) {
            if (C[j] == (uint32_t)tid) {
                const float f = __uint_as_float(F[j]);
                n += 1;
                mk = max(mk, rm_score_key(f));
                if (f == f) sum += (double)f;
            }
        }
        const int64_t o = (int64_t)blockIdx.x * kRmCats + tid;
        a.cat_n[o] = n;
        a.cat_max[o] = n ? rm_key_score(mk) : 0.0f;
        a.cat_sum[o] = sum;
    }
}

struct MmArgs {
    const int32_t *ranked, *count, *node, *eid;
    int32_t rows, k, ne, n_m, max_m;
    int32_t m[kRmMaxM];
    int32_t *out;
};

// one workgroup per row: the ids of its first min(max m, count, k) triples in LDS; a slot finds the first triple that
// holds its edge id and is kept by every m above that triple's rank
__global__ void __launch_bounds__(256) motif_mask_kernel(MmArgs a) {
    extern __shared__ int32_t mm_lds[];                       // [3 * max_m]
    const int row = blockIdx.x, tid = threadIdx.x;
    const int top = max(0, min(a.max_m, min(a.count[row], a.k)));
    for (int t = tid; t < 3 * top; t += 256) mm_lds[t] = a.ranked[(int64_t)row * a.k * 3 + t];
    __syncthreads();
    for (int s = tid; s < a.ne; s += 256) {
        const int64_t o = (int64_t)row * a.ne + s;
        const int32_t nd = a.node[o], e = a.eid[o];
        int first = top;                                      // rank of the first triple holding e; top: none
        if (nd != 0 && e > 0)
            for (int t = 3 * top - 1; t >= 0; --t)
                if (mm_lds[t] == e) first = t / 3;
        for (int g = 0; g < a.n_m; ++g)
            a.out[((int64_t)g * a.rows + row) * a.ne + s] = first < min(a.m[g], top) ? nd : 0;
    }
}

}  // namespace tmk

using namespace tmk;

extern "C" int tm_ranked_motifs(const int32_t *eid3, const int32_t *cat, const float *imp, int32_t rows, int32_t W,
                                const int32_t *group_rows, int32_t n_groups, int32_t rows_per_group, int32_t k,
                                int32_t *out_eid, float *out_score, int32_t *out_walk, int32_t *out_mult,
                                int32_t *out_cat, int32_t *out_count, int32_t *cat_n, float *cat_max, double *cat_sum,
                                int32_t *err_flag, void *stream) {
    if (rows < 0 || W < 1 || n_groups < 0 || (rows_per_group != 1 && rows_per_group != 2))
        return fail(TM_E_ARG, "tm_ranked_motifs: rows >= 0, W >= 1, n_groups >= 0 and 1 or 2 rows per group are "
                              "required");
    const int64_t total = (int64_t)W * rows_per_group;
    if (total > kRmMaxEntries)
        return fail(TM_E_UNSUPPORTED, "tm_ranked_motifs: " + std::to_string(total) + " entries per group (" +
                                          std::to_string(rows_per_group) + " rows of " + std::to_string(W) +
                                          " walks) exceed the limit of " + std::to_string(kRmMaxEntries));
    if (k < 1 || k > total)
        return fail(TM_E_ARG, "tm_ranked_motifs: k = " + std::to_string(k) + " is outside [1, " +
                                  std::to_string(total) + "], the entries of a group");
    if (n_groups == 0) return TM_OK;
    if (!eid3 || !cat || !imp || !group_rows || !out_eid || !out_score || !out_walk || !out_mult || !out_cat ||
        !out_count || !cat_n || !cat_max || !cat_sum)
        return fail(TM_E_ARG, "tm_ranked_motifs: NULL pointer");
    const RmArgs a{eid3, cat, imp, group_rows, rows, W, rows_per_group, k, out_eid, out_score, out_walk, out_mult,
                   out_cat, out_count, cat_n, cat_max, cat_sum, err_flag};
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t pe = prof_begin(s);
    const int T = ((int)total + 63) / 64 * 64;                // whole waves; 40 bytes of LDS per thread, 40 KB at most
    const size_t lds = (size_t)T * 40 + (size_t)(T / 64) * 4;
    ranked_motifs_kernel<<<dim3((unsigned)n_groups), T, lds, s>>>(a);
    TM_CHECK_LAUNCH();
    prof_end("ranked_motifs_kernel", s, pe);
    return TM_OK;
}

extern "C" int tm_motif_mask(const int32_t *ranked_eid, const int32_t *count, int32_t rows, int32_t k,
                             const int32_t *node, const int32_t *eid, int32_t ne, const int32_t *m_list, int32_t n_m,
                             int32_t *node_out, void *stream) {
    if (rows < 0 || k < 1 || k > kRmMaxEntries || ne < 1 || n_m < 1 || n_m > kRmMaxM || !m_list)
        return fail(TM_E_ARG, "tm_motif_mask: rows >= 0, k in [1, " + std::to_string(kRmMaxEntries) +
                                  "], ne >= 1 and 1 to " + std::to_string(kRmMaxM) + " values of m are required");
    MmArgs a{ranked_eid, count, node, eid, rows, k, ne, n_m, 0, {}, node_out};
    for (int g = 0; g < n_m; ++g) {
        if (m_list[g] < 1 || m_list[g] > k)
            return fail(TM_E_ARG, "tm_motif_mask: m = " + std::to_string(m_list[g]) + " is outside [1, " +
                                      std::to_string(k) + "], the ranked motifs of a row");
        a.m[g] = m_list[g];
        a.max_m = std::max(a.max_m, m_list[g]);
    }
    if (rows == 0) return TM_OK;
    if (!ranked_eid || !count || !node || !eid || !node_out) return fail(TM_E_ARG, "tm_motif_mask: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t pe = prof_begin(s);
    motif_mask_kernel<<<dim3((unsigned)rows), 256, (size_t)a.max_m * 12, s>>>(a);
    TM_CHECK_LAUNCH();
    prof_end("motif_mask_kernel", s, pe);
    return TM_OK;
}
