// Encoder internals shared by encoder.hip (scoring) and encoder_train.hip (training forward/backward).
#pragma once
#include <vector>

#include "common.h"

typedef float floatx4 __attribute__((ext_vector_type(4)));

namespace tmk {

constexpr int HID = 64;   // hid_dim supported by this build (reference default --hid_dim 64)
constexpr int TILE_ROWS = 32;
constexpr size_t LDS_BUDGET = 160 * 1024;   // bytes of LDS one workgroup may ask for (a CDNA4 CU's 160 KB)

__host__ __device__ constexpr int r16(int x) { return (x + 15) & ~15; }

struct Lin {
    const float4 *w;  // packed [nt][nq][64 lanes] float4
    const float *b;   // [nt*16] zero padded
    int nt, nq, nout, k;
};

struct EncW {
    int de, dn, kev, kdep;
    Lin ev, g1, g2, w1, w2, a1, a2, m1, m2, d1, d2;
    const float *m3w, *m3b, *d3w, *d3b, *freq, *phase;
    // lin_event bias plus the K steps q >= qt (all time features) at dt = 0: walk position 2 is
    // relative to itself, so those steps are the constant cos(phase) (walk_kernel's slot pass)
    const float *evc;
    int qt;   // in the walk kernel's 32-wide K steps: (de + 3 + 31) / 32
    // lin_event's weights for the walk kernel's bf16 MFMA form (split3), tile-major: per (output tile t, K step s,
    // part hi / mid / lo) one fragment, the steps of a tile and the parts of a step one after the other
    // (Ev3Lay: its sizes and offsets).  ns3 = ceil(kev / 32) steps.  A 32-wide step's fragment is 1 KB in
    // v_mfma_f32_16x16x32_bf16's A-operand lane order: lane l holds row 16t + (l & 15), k = 32s + 8(l >> 4) + 0..7.
    // When 1 <= kev mod 32 <= 16 the last step is 16 deep instead (ev3_tail), its fragments 512 B in
    // v_mfma_f32_16x16x16_bf16's A-operand lane order: lane l holds row 16t + (l & 15), k = 32s + 4(l >> 4) + 0..3.
    // Rows >= dn and k >= kev are zero.  In tm_weights::buf, so one buffer resource reaches it.
    const float4 *ev3;
    int ns3;
    // event_gcn's first layer (g1) for the zero-node walk kernel's bf16 MFMA form, split3 like ev3: per (output
    // tile t, pair step u, part) one 1 KB fragment at float4 offset ((t * nsg + u) * 3 + part) * 64.  A pair step
    // spans the input tiles 2u and 2u + 1 in the D-tile lane order lin_event leaves them in: lane l (row
    // 16t + (l & 15), group g = l >> 4) holds W[row][gcn_split_col(u, g, j)], j = 0..7; zero for a column >= dn
    // (the padding of the last tile, and with an odd tile count the whole second half of the last step).
    const float4 *g13;
    int nsg;   // pair steps: (r16(dn) / 16 + 1) / 2
    // lin_event's folded time steps alone (evc - bias, fp64 sum rounded once): the table-mode slot pass,
    // whose edge-table row already carries the bias
    const float *devc;
    // fused walk kernel (eval, hid_dim 64): layers folded at pack time in fp64 (tm_weights_pack).  With
    // H = event_gcn's relu'd hidden layer of both branches, F = blockdiag(g2, g2) H + [bg2; bg2];
    // W1D = W1 blockdiag(g2,g2), b1d = W1 [bg2;bg2] + b1 (so Wp = W1 F_2 + b1 = W1D H_2 + b1d),
    // G = W2 blockdiag(g2,g2), beta = W2 [bg2;bg2] + b2 (Q_i = W2 F_i + b2 = G H_i + beta).  The score
    // Wp . Q_i = V . H_i + cw with V = G^T Wp = kv H_2 + v0 (kv = G^T W1D, v0 = G^T b1d) and
    // cw = Wp . beta = u . H_2 + c0 (u = W1D^T beta, c0 = b1d . beta); attention.MLP.0 of the
    // attention output = P2 + A1G (alpha_0 H_0 + alpha_1 H_1) with P2 = A1D H_2 + cp
    // (A1D = a1 blockdiag(g2,g2), A1G = a1 G, cp = a1 [bg2;bg2] + a1 beta + ba1; alpha_0 + alpha_1 = 1);
    // M1A2 = MLP.0[:, :h] a2, tc[c] = MLP.0[:, h + c] + bm1 + MLP.0[:, :h] ba2 (row 12: no category).
    Lin kv, a1d, a1g, m1a2;
    const float *v0, *u, *c0, *cp, *tc;
    // zero node features (tm_weights_set_node_zero; FoldLay KVZ ...): the same layers on U = H[:64] = H[64:]
    Lin kvz, a1dz, a1gz;
    const float *v0z, *uz;
    // constructor variants (explainer_new.py:103-105, :121, :141): tg = use_temporal_guidance (0: the plain
    // Attention, no time weighting of the scores), dep = use_dependency_aware_sampling (0: no gate)
    int tg = 1, dep = 1;
    // hid_dim and the final MLP's width (hm = h + 12 with the one-hot category feature, h without:
    // if_cat_feature, explainer_new.py:121-125); the fused walk kernel covers h = 64 with the category
    int h = 64, hm = 76, cat = 1;
};

// ------------------------------------------------------------------ MFMA tile GEMM
// out[16mt.., 16nt..] = X[16*MT rows][ldx] (LDS) * W^T (packed, streamed from L2).
// Each wave owns column tiles nt = wave, wave + nw, ... and sweeps all MT row tiles for
// them, two column tiles at a time: per 16-deep K step it loads 2 weight fragments (the
// next step's are prefetched into registers) and MT activation fragments (ds_read_b128)
// and issues 8*MT MFMAs.  The epilogue gets (mt, nt, acc) with acc[r] = D[4*(lane>>4)+r][lane&15].
template <int MT, class Epi>
__device__ __forceinline__ void gemm(const float *X, int ldx, const Lin &L, Epi epi) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int arow = lane & 15, akoff = 4 * (lane >> 4);
    const int nq = L.nq;
    for (int nt0 = wave; nt0 < L.nt; nt0 += 2 * nw) {
        const int nt1 = nt0 + nw;
        const bool has1 = nt1 < L.nt;
        floatx4 acc0[MT], acc1[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            acc0[m] = floatx4{0.f, 0.f, 0.f, 0.f};
            acc1[m] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
        const float4 *wb0 = L.w + (size_t)nt0 * nq * 64 + lane;
        const float4 *wb1 = L.w + (size_t)(has1 ? nt1 : nt0) * nq * 64 + lane;
        const float *xa = X + arow * ldx + akoff;
        float4 b0 = wb0[0], b1 = wb1[0];
        for (int q = 0; q < nq; ++q) {
            float4 n0 = b0, n1 = b1;
            if (q + 1 < nq) {
                n0 = wb0[(q + 1) * 64];
                n1 = wb1[(q + 1) * 64];
            }
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const float4 a = *reinterpret_cast<const float4 *>(xa + m * 16 * ldx + 16 * q);
                acc0[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b0.x, acc0[m], 0, 0, 0);
                acc1[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b1.x, acc1[m], 0, 0, 0);
                acc0[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b0.y, acc0[m], 0, 0, 0);
                acc1[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b1.y, acc1[m], 0, 0, 0);
                acc0[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b0.z, acc0[m], 0, 0, 0);
                acc1[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b1.z, acc1[m], 0, 0, 0);
                acc0[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b0.w, acc0[m], 0, 0, 0);
                acc1[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b1.w, acc1[m], 0, 0, 0);
            }
            b0 = n0;
            b1 = n1;
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) epi(m, nt0, acc0[m]);
        if (has1) {
#pragma unroll
            for (int m = 0; m < MT; ++m) epi(m, nt1, acc1[m]);
        }
    }
}

__device__ __forceinline__ int erow(int mt, int r) { return mt * 16 + 4 * ((threadIdx.x & 63) >> 4) + r; }
__device__ __forceinline__ int ecol(int nt) { return nt * 16 + (threadIdx.x & 15); }

// cos(t * w + phi) with the multiply and add rounded separately, as torch does
// (TimeEncode.forward, explainer_new.py:56-58); never contracted into an fma (time_arg, common.h).
__device__ __forceinline__ float time_cos(float t, float w, float phi) { return cos_rd(time_arg(t, w, phi)); }
// the derivative's sine at the same argument
__device__ __forceinline__ float time_sin(float t, float w, float phi) { return sin_rd(time_arg(t, w, phi)); }
// the temporal attention's score multiplier 1.0 - 0.3 + 0.3 * time_weight (explainer_new.py:835-836): 0.7 in
// fp32, a rounded product, a rounded sum
__device__ __forceinline__ float tw_mult(float tw) { return time_arg(0.3f, tw, 0.7f); }

__device__ __forceinline__ float relu(float x) { return x > 0.f ? x : 0.f; }

// ------------------------------------------------------------------ exact three-way bf16 split of an fp32 value
// bf16 bit pattern of v rounded to nearest even; a finite v whose round-up would reach the infinity pattern
// truncates instead (stays the largest finite bf16), NaN keeps a mantissa bit
__host__ __device__ inline uint16_t bf16_rne_bits(float v) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)((u >> 16) | ((u & 0xffffu) ? 0x40u : 0u));
    const uint32_t r = (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
    return (uint16_t)((r & 0x7f80u) == 0x7f80u ? (u >> 16) : r);
}
__host__ __device__ inline float bf16_bits_f32(uint16_t b) { return __builtin_bit_cast(float, (uint32_t)b << 16); }
// v = hi + mid + lo (micro/split.hip's split8, one element): both residuals are exact fp32 differences, and the
// last one fits bf16's 8 bits whenever it stays above bf16's denormal step (|v| >= 2^-110); non-finite v: hi alone
__host__ __device__ inline void split3(float v, uint16_t &hi, uint16_t &mid, uint16_t &lo) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    hi = bf16_rne_bits(v);
    mid = lo = 0;
    if ((u & 0x7f800000u) == 0x7f800000u) return;
    const float r1 = v - bf16_bits_f32(hi);
    // hi truncated (the top binade's last bf16 step): mid truncates too, or hi + mid would round up to inf
    const bool trunc = (hi & 0x7fffu) == 0x7f7fu && (u & 0xffffu) >= 0x8000u;
    mid = trunc ? (uint16_t)(__builtin_bit_cast(uint32_t, r1) >> 16) : bf16_rne_bits(r1);
    lo = bf16_rne_bits(r1 - bf16_bits_f32(mid));
    // a zero part takes the value's sign, so that -0 = (-0) + (-0) + (-0) bit for bit
    if ((mid & 0x7fffu) == 0) mid = hi & 0x8000u;
    if ((lo & 0x7fffu) == 0) lo = hi & 0x8000u;
}

// input feature in K slot (lane group g, element j) of pair step u of the g1 split pack (EncW::g13): elements 0..3
// from input tile 2u, 4..7 from tile 2u + 1, each lane's 4 rows of the f32 D-tile layout
__host__ __device__ constexpr int gcn_split_col(int u, int g, int j) { return 16 * (2 * u + (j >> 2)) + 4 * g + (j & 3); }
// column of element (K step s, lane group g, element j) of a split pack: mode 1 = ev3 (plain 32-wide steps; deep16:
// its 16-deep last step, 4 elements per lane), mode 2 = g13 (pair steps)
__host__ __device__ constexpr int split_pack_col(int mode, int s, int g, int j, bool deep16 = false) {
    return mode == 2 ? gcn_split_col(s, g, j) : deep16 ? 32 * s + 4 * g + j : 32 * s + 8 * g + j;
}
// EncW::ev3 ends in a 16-deep step when the last 32-wide step would hold at most 16 real features
__host__ __device__ constexpr bool ev3_tail(int kev) { return ((kev - 1) & 31) < 16; }
// EncW::ev3 in bf16 units: a tile's nf 32-wide steps (3 x 512 each), then its 16-deep step (3 x 256) if it has one
struct Ev3Lay {
    int nf, tail;   // 32-wide steps; 1: a 16-deep step follows them
    __host__ __device__ constexpr Ev3Lay(int ns3, bool t) : nf(ns3 - (t ? 1 : 0)), tail(t ? 1 : 0) {}
    __host__ __device__ constexpr int tile() const { return nf * 1536 + tail * 768; }   // bf16 per output tile
    __host__ __device__ constexpr int elems() const { return nf * 512 + tail * 256; }   // weights per output tile
    // fragment (tile t, step s, part) -> its first bf16 (s == nf: the 16-deep step)
    __host__ __device__ constexpr int frag(int t, int s, int part) const {
        return t * tile() + (s < nf ? (s * 3 + part) * 512 : nf * 1536 + part * 256);
    }
};
// weight e of the pack's tile-major enumeration (e < tiles * elems()) -> its row o and column c in W and its hi
// part's bf16 index d; the mid and lo parts follow at d + ps and d + 2 ps
__host__ __device__ inline void ev3_elem(const Ev3Lay &L, int64_t e, int &o, int &c, int64_t &d, int &ps) {
    const int t = (int)(e / L.elems()), r = (int)(e % L.elems());
    const bool deep16 = r >= L.nf * 512;
    const int s = deep16 ? L.nf : r >> 9, q = deep16 ? r - L.nf * 512 : r & 511;
    const int l = deep16 ? q >> 2 : q >> 3, j = deep16 ? q & 3 : q & 7;
    o = 16 * t + (l & 15);
    c = split_pack_col(1, s, l >> 4, j, deep16);
    ps = deep16 ? 256 : 512;
    d = (int64_t)L.frag(t, s, 0) + q;
}

// The dependency gate's logit d3 . G2 over its h2 = h/2 features in ONE fixed order, shared by the
// LDS-tiled kernels and the register-resident gate_reg_kernel (h2 = 32) so their gates agree bit for bit:
// part k (k = 0..3) is an fma chain over features 16t + 4k + r (t < h2/16 rounded up, r = 0..3) and
// z = (part0 + part1) + (part2 + part3).
__device__ __forceinline__ float gate_part(const float *g2, const float *w3, int k, int h2 = 32) {
    float p = 0.f;
    for (int t = 0; 16 * t < h2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) p = __builtin_fmaf(g2[16 * t + 4 * k + r], w3[16 * t + 4 * k + r], p);
    return p;
}
// LDS form: 8 lanes per row (sub = lane & 7), the row's relu'd G2 at g2 (zero padded to a multiple of 16;
// w3 likewise); the result in every lane
__device__ __forceinline__ float gate_logit_lds(const float *g2, const float *w3, int sub, int h2 = 32) {
    float v = sub < 4 ? gate_part(g2, w3, sub, h2) : 0.f;
    v += __shfl_xor(v, 1, 8);
    v += __shfl_xor(v, 2, 8);
    return v;
}

// Folded region at the start of tm_weights::buf (float offsets; hid_dim 64): the fused walk kernel's
// packs and vectors (EncW::w1d ...), then the reference layers in tm_weights_create's order.
struct FoldLay {
    static constexpr int KV = 0, V0 = KV + 8 * 8 * 256, U = V0 + 128, C0 = U + 128, A1D = C0 + 4, CP = A1D + 4 * 8 * 256,
                         A1G = CP + 64, M1A2 = A1G + 4 * 8 * 256, TC = M1A2 + 5 * 4 * 256,
                         // the zero-node-feature forms (H_s = H_t = U, so H = [U; U] and every layer reading H
                         // takes the sum of its two column halves; kv and v0 also sum their two row halves, the
                         // score V . H_i becoming VZ . U_i with VZ = V[:64] + V[64:])
                         KVZ = (TC + 13 * 80 + 63) & ~63, A1DZ = KVZ + 4 * 4 * 256, A1GZ = A1DZ + 4 * 4 * 256,
                         V0Z = A1GZ + 4 * 4 * 256, UZ = V0Z + 64, SIZE = (UZ + 64 + 63) & ~63;
    // fold32 scratch (row-major fp32 matrices before packing)
    static constexpr int S_KV = 0, S_A1D = S_KV + 128 * 128, S_A1G = S_A1D + 64 * 128, S_M1A2 = S_A1G + 64 * 128,
                         S_KVZ = S_M1A2 + 76 * 64, S_A1DZ = S_KVZ + 64 * 64, S_A1GZ = S_A1DZ + 64 * 64,
                         S_SIZE = S_A1GZ + 64 * 64;
    // fold64 scratch (stage 1): a1 W2, a1 b2, W1D = W1 blockdiag(g2,g2), G = W2 blockdiag(g2,g2), b1d, beta
    static constexpr int S64_A1W2 = 0, S64_A1B2 = S64_A1W2 + 64 * 128, S64_W1D = S64_A1B2 + 64,
                         S64_G = S64_W1D + 128 * 128, S64_B1D = S64_G + 128 * 128, S64_BETA = S64_B1D + 128,
                         S64_SIZE = S64_BETA + 128;
};

// Transposed weight packs for the backward's data-gradient GEMMs (dX = dY W = dY (W^T)^T), same
// fragment format as the forward packs; no biases.  evT holds only lin_event's time-feature columns.
struct EncWT {
    Lin evT, g1T, g2T, w1T, w2T, a1T, a2T, m1T, m2T;
    Lin d1T, d2T;   // dependency gate: d1T holds only the time-feature columns of edge_dependency_gcn.0
};

// Dropout keep-masks of the training forward, uint8 [n_walks][drop_cols(h, hm)]: attention weights alpha
// (TemporalAwareAttention.dropout, explainer_new.py:839) in columns 0..1, the attention MLP's hidden layer
// (:780) in the h columns from DROP_H and the final MLP's hidden layer (:122) in the hm columns from
// DROP_H + h; 1 = kept (scaled by 1/(1-p)), 0 = dropped.  Rows padded to 16 columns (144 for the default
// hid_dim 64 with the category feature).  The plain Attention (use_temporal_guidance=False, :12-43) has
// neither of the first two dropouts: their columns are ignored then.
constexpr int DROP_A = 0, DROP_H = 2;
__host__ __device__ constexpr int drop_cols(int h, int hm) { return r16(DROP_H + h + hm); }
static_assert(drop_cols(HID, HID + 12) == 144, "dropout mask columns");

// ------------------------------------------------------------------ register-resident MFMA chains (shared by the
// fused walk kernel and the register-resident training kernels)
// out[t] = W tile t * x  over the flattened (t, q) sequence, weights prefetched PF steps ahead in
// a rotating register buffer; sched_barrier pins each step so the loads stay PF steps ahead instead
// of being hoisted (which would need NTO*NQ registers).
constexpr int PF = 3;

// The lane index laundered through an opaque asm: loads addressed with it cannot be hoisted out of
// the pass loop by LICM (hoisting every loop-invariant weight/bias load costs ~300 registers).
__device__ __forceinline__ int lane_id() {
    int l = threadIdx.x & 63;
    asm volatile("" : "+v"(l));
    return l;
}

// Weight fragments are read with buffer loads: the fragment's byte offset is a compile-time SGPR
// operand (s_mov, scalar pipe) instead of a 64-bit VGPR address add per fragment.  The lane offset
// goes through lane_id() so the loads stay inside the pass loop.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wrsrc(const float4 *w) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float4 *>(w), (short)0, 0x7fffffff, 0x00020000);
}

__device__ __forceinline__ float4 wload(__amdgpu_buffer_rsrc_t r, int vo, int f4) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, vo, f4 * 16, 0));
}

template <int NTO, int NQ>
struct PairOrder {   // fragment i of the pair order -> (tile, K step)
    static constexpr int NP = NTO / 2, NPF = 2 * NP * NQ;
    static constexpr int t(int i) { return i < NPF ? 2 * (i / (2 * NQ)) + (i & 1) : NTO - 1; }
    static constexpr int q(int i) { return i < NPF ? (i % (2 * NQ)) / 2 : i - NPF; }
};

// NQL = the pack's K steps (L.nq); NQ <= NQL of them are multiplied (the leading ones).  Tile pairs (t, t+1)
// with their K steps inside and the two tiles' MFMAs interleaved (no MFMA waits on the accumulator of the one
// before it: 32-cycle issue, 40-cycle dependent latency); an odd last tile alone.  Every tile accumulates its
// K steps in the same order as a tile-by-tile loop (same results).
template <int NTO, int NQ, int NQL = NQ>
__device__ __forceinline__ void rgemm(const Lin &L, const floatx4 (&x)[NQ], floatx4 (&o)[NTO]) {
    using O = PairOrder<NTO, NQ>;
    const auto wr = wrsrc(L.w);
    const int vo = lane_id() * 16;
    constexpr int N = NTO * NQ, D = PF < N ? PF : N;
    auto off = [](int i) { return (O::t(i) * NQL + O::q(i)) * 64; };
#pragma unroll
    for (int t = 0; t < NTO; ++t) o[t] = floatx4{0.f, 0.f, 0.f, 0.f};
    float4 buf[D];
#pragma unroll
    for (int i = 0; i < D; ++i) buf[i] = wload(wr, vo, off(i));
#pragma unroll
    for (int k = 0; k < O::NP * NQ; ++k) {
        const int i = 2 * k, t = O::t(i), q = O::q(i);
        const float4 w0 = buf[i % D];
        if (i + D < N) buf[i % D] = wload(wr, vo, off(i + D));
        const float4 w1 = buf[(i + 1) % D];
        if (i + 1 + D < N) buf[(i + 1) % D] = wload(wr, vo, off(i + 1 + D));
        o[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.x, x[q].x, o[t], 0, 0, 0);
        o[t + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.x, x[q].x, o[t + 1], 0, 0, 0);
        o[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.y, x[q].y, o[t], 0, 0, 0);
        o[t + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.y, x[q].y, o[t + 1], 0, 0, 0);
        o[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.z, x[q].z, o[t], 0, 0, 0);
        o[t + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.z, x[q].z, o[t + 1], 0, 0, 0);
        o[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.w, x[q].w, o[t], 0, 0, 0);
        o[t + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.w, x[q].w, o[t + 1], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (NTO % 2) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int i = O::NPF + q;
            const float4 w = buf[i % D];
            if (i + D < N) buf[i % D] = wload(wr, vo, off(i + D));
            o[NTO - 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, x[q].x, o[NTO - 1], 0, 0, 0);
            o[NTO - 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, x[q].y, o[NTO - 1], 0, 0, 0);
            o[NTO - 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, x[q].z, o[NTO - 1], 0, 0, 0);
            o[NTO - 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, x[q].w, o[NTO - 1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// the register-resident event_gcn forward of the training step (encoder_train.hip) for these dims: launched
// on s (true), or no instance (false: the caller runs gcn_kernel)
bool launch_gcn_fwd_reg(const EncW &P, int node_zero, int64_t n_rows, const float *n_feat, const float *e_feat, const int32_t *node6,
                        const int32_t *eid3, const float *ts3, const float *cnt, float *F, hipStream_t s);

// log2 of the explanation kernels' LDS hash size: at least 64 slots, and twice an event's 3 W walk positions
inline int expl_hbits(int W) {
    int hbits = 6;
    while ((1 << hbits) < 2 * 3 * W) ++hbits;
    return hbits;
}

// enhance.hip: the pooled encoder's tail, one workgroup per (group, event): out[e][0:h] = a2 (sum of the event's
// n_part partial rows of `part`, in a fixed order) + a2.b * (sum of its W walk weights, in order), and with do_cat
// out[e][h:h+12] = the event's category histogram
void launch_pool_tail(const Lin &a2, int64_t n_events, int32_t W, int32_t n_part, int32_t h, int32_t do_cat,
                      const float *part, const float *wgt, const int32_t *cat, float *out, int64_t ld_out,
                      hipStream_t s);

}  // namespace tmk

using tmk::Lin;
using tmk::EncW;

struct tm_weights {
    int device;
    int de, dn, h;
    float *buf;
    size_t n_floats;
    EncW P;
    // the caller's node-feature table is all zeros (tm_weights_set_node_zero): the fused eval kernel computes
    // one event_gcn branch, the other being bit-identical
    int node_zero = 0;
    // a process-wide stamp (tm_weights_bump: every create / repack / variant / node-zero change takes the next
    // value of one global counter): caches of values computed from the weights (the drop-in's gate factors per
    // edge id, the pipeline's per-edge-id tables) key on it, and no two weight states -- of this object or of
    // another one later allocated at the same address -- ever share a stamp
    uint64_t version = 0;
    // per linear: raw tensor index, nout, k
    struct Spec {
        Lin *lin;
        int wi, nout, k;
    };
    std::vector<Spec> specs;
    std::vector<std::pair<int, float **>> vecs;
    // training: transposed packs (encoder_train.hip)
    tmk::EncWT T;
    float *tbuf = nullptr;
    size_t t_floats = 0;
    // fold scratch (tm_weights_pack): fp64 a1 W2 [h][2h] and fp32 row-major folded matrices before packing
    double *fold64 = nullptr;
    float *fold32 = nullptr;
};

void tm_weights_bump(tm_weights *w);   // encoder.hip: w->version = the next process-wide stamp

// The encoder's workspace, written by the forwards and read back by tm_encoder_bwd / tm_encoder_pool_bwd:
//   F [n_walks][3][2h] | the groups' std (n_walks + 64 floats) | 256 spare bytes
// and for the pooled forwards, from the next multiple of 256 bytes on:
//   the partial rows [n_walks][h] (the fused kernel uses n_slots * PM <= n_walks of them) | 256 spare bytes
// The fused walk kernel leaves F unused and keeps the unit counter of its persistent launch in F's first word.
struct EncWsLay {   // byte offsets from the workspace's start
    int64_t stdv, bytes, part, pool_bytes;
};
inline EncWsLay enc_ws_lay(const tm_weights *w, int64_t n_walks) {
    const int64_t h = w ? w->h : tmk::HID, f = sizeof(float);
    EncWsLay l;
    l.stdv = n_walks * 3 * 2 * h * f;
    l.bytes = l.stdv + (n_walks + 64) * f + 256;
    l.part = (l.bytes + 255) & ~(int64_t)255;
    l.pool_bytes = l.part + n_walks * h * f + 256;
    return l;
}
struct EncWs {
    float *F, *stdv;
    uint32_t *ticket;
    float *part;   // only in a workspace of the pooled size
};
inline EncWs enc_ws(const tm_weights *w, int64_t n_walks, void *workspace) {
    const EncWsLay l = enc_ws_lay(w, n_walks);
    char *p = static_cast<char *>(workspace);
    return {reinterpret_cast<float *>(p), reinterpret_cast<float *>(p + l.stdv), reinterpret_cast<uint32_t *>(p),
            reinterpret_cast<float *>(p + l.part)};
}

// encoder_train.hip: transposed packs (tm_weights_create / _free) and the one-launch packing of every tensor
int train_packs_create(tm_weights *w);
void pack_all_weights(tm_weights *w, const float *const *t, hipStream_t s);   // every pack, one launch (+ evc)
void train_packs_free(tm_weights *w);

static inline hipStream_t S_(void *s) { return (hipStream_t)s; }
