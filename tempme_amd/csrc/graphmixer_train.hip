// Training of the base GraphMixer's node embeddings on gfx950 (learn_base.py with --base_type graphmixer):
// the forward of compute_node_temporal_embeddings (GraphM/graphmixer.py:142-193, :244-315) with the four
// dropouts of every mixer layer, and the gradient of every trainable embedding parameter.  explain_weights
// and edge_attr are None here (learn_base.py:228-232 passes neither).
//
//   gt_fwd_kernel        one workgroup (4 waves) per row: projection, L mixer layers, masked token mean,
//                        neighbour mean.  Writes the projection input F and every layer's input image X_l to
//                        the workspace; nothing else is kept.
//   gt_bwd_layer_kernel  one launch per layer, last layer first, one workgroup per row: reloads X_l, recomputes
//                        the layer's forward (same masks), runs the activation-gradient chain and emits the
//                        operand images of the layer's weight gradients (dZ, LN outputs, hidden activations)
//                        as [R N][ld] / [R C][ld] matrices; the row's d X_l goes back to the workspace for the
//                        next launch.  LDS holds one layer at a time, so the footprint does not grow with L.
//   tm_wgrad             (encoder_train.hip) reduces the images: 8 jobs per layer, one for the projection;
//                        fixed-order two-stage reduction, so the gradients are deterministic.  LayerNorm
//                        parameter gradients are column sums of images (dY * xhat, dY): jobs with a
//                        one-column X whose weight output goes to a scratch row.
//
// GEMMs (projection, channel FFN and its two transposes) are fp32 MFMA 16x16x4 with the activations as the A
// operand from LDS (one float4 per lane per 16-wide K block: the lane's four K values feed four MFMAs, the B
// operand loaded with the same K assignment) and the weights as the B operand straight from their row-major
// nn.Linear layout in global memory (float4 when the row stride allows it), so no weight pack is rebuilt
// after an optimizer step; the backward's two transposed operands are plain transposed copies.  Token mixing
// (N <= 32 tokens, HT <= 16 hidden) is one thread per channel on the VALU, its weights zero-padded in LDS.
#include <algorithm>

#include "common.h"
#include "gm_common.h"

namespace tmk {

typedef float gtx4 __attribute__((ext_vector_type(4)));

constexpr int GT_MT = 32;      // tokens per row (two 16-row MFMA tiles)
constexpr int GT_HTP = 16;     // token-FFN hidden units, padded
constexpr int GT_HCH = 128;    // channel-FFN hidden features per LDS chunk (8 tiles: 2 per wave)
constexpr int GT_MAXL = 4;
constexpr int GT_TOKW = 2 * GT_MT + 2 * GT_MT * GT_HTP + GT_HTP + GT_MT;   // token LN + FFN weights in LDS
constexpr int GT_DUMMY = 4 * 256;   // scratch weight outputs of the LayerNorm column-sum jobs

struct GtArgs {
    int32_t R, N, C, T, D, L, HT, HC;
    const int32_t *node, *nid, *eid;
    const double *cut, *ts;
    const float *n_feat, *e_feat, *time_w, *time_b, *proj_w, *proj_b;
    const float *const *lw;   // [L][14] device table
    const uint8_t *keep;      // per layer: tok_h [R][C][HT], tok_o [R][C][N], ch_h [R][N][HC], ch_o [R][N][C]
    float keep_scale;
    float *x_mean, *node_out;
    float *ws;
};

__host__ __device__ inline int32_t gt_r4(int32_t x) { return (x + 3) & ~3; }

// workspace layout (floats); every offset is a multiple of 4 floats
struct GtWs {
    int64_t F, XL, DX, Yc, dYc, Gc, dOc, Hc, dHc, Yt, dYt, Gt, dOt, Ht, dHt, dummy, total;
    int32_t ldC, ldK, ldH;
};
__host__ __device__ inline GtWs gt_ws(int64_t R, int N, int C, int T, int L, int HC) {
    GtWs w;
    w.ldC = gt_r4(C);
    w.ldK = gt_r4(C + T);
    w.ldH = gt_r4(HC);
    const int64_t RN = R * N, RC = R * C;
    int64_t o = 0;
    w.F = o;     o += RN * w.ldK;
    w.XL = o;    o += (int64_t)L * RN * w.ldC;
    w.DX = o;    o += RN * w.ldC;
    w.Yc = o;    o += RN * w.ldC;
    w.dYc = o;   o += RN * w.ldC;
    w.Gc = o;    o += RN * w.ldC;
    w.dOc = o;   o += RN * w.ldC;
    w.Hc = o;    o += RN * w.ldH;
    w.dHc = o;   o += RN * w.ldH;
    w.Yt = o;    o += RC * GT_MT;
    w.dYt = o;   o += RC * GT_MT;
    w.Gt = o;    o += RC * GT_MT;
    w.dOt = o;   o += RC * GT_MT;
    w.Ht = o;    o += RC * GT_HTP;
    w.dHt = o;   o += RC * GT_HTP;
    w.dummy = o; o += GT_DUMMY;
    w.total = o;
    return w;
}

// bytes of one layer's keep masks, and the offsets of its four parts
struct GtKeep {
    int64_t tok_h, tok_o, ch_h, ch_o, layer;
};
__host__ __device__ inline GtKeep gt_keep(int64_t R, int N, int C, int HT, int HC) {
    GtKeep k;
    k.tok_h = 0;
    k.tok_o = k.tok_h + R * C * HT;
    k.ch_h = k.tok_o + R * C * N;
    k.ch_o = k.ch_h + R * N * HC;
    k.layer = k.ch_o + R * N * C;
    return k;
}

// dropout factor of element i: keep_scale when kept, 0 when dropped, 1 without masks
__device__ __forceinline__ float gt_kf(const uint8_t *keep, int64_t i, float scale) {
    return keep ? (keep[i] ? scale : 0.f) : 1.f;
}

// columns k .. k+3 of a weight row of K columns (zero past the end)
__device__ __forceinline__ float4 gt_ld4(const float *row, int k, int K, bool vec) {
    if (vec && k + 3 < K) return *reinterpret_cast<const float4 *>(row + k);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k < K) v.x = row[k];
    if (k + 1 < K) v.y = row[k + 1];
    if (k + 2 < K) v.z = row[k + 2];
    if (k + 3 < K) v.w = row[k + 3];
    return v;
}

// acc[i][q][e] += sum_k A[16 q + 4 (lane / 16) + e][k] * W[16 (t0 + 4 i) + lane % 16][k] for the wave's output
// tiles t0 + 4 i (i < ntw): A an LDS image [32][lda] with KB 16-wide K blocks (zero past K), W row-major
// [J][ldw] in global memory with K used columns.  Rows of W past J read as zero.
template <int NTW>
__device__ __forceinline__ void gt_gemm(const float *A, int lda, int KB, const float *W, int ldw, int J, int K,
                                        bool vec, int t0, int ntw, gtx4 (&acc)[NTW][2]) {
    const int lane = threadIdx.x & 63, m = lane & 15, q = lane >> 4;
    vec = vec && (reinterpret_cast<uintptr_t>(W) & 15) == 0;   // a parameter may be a view at any offset of a bucket
    for (int g = 0; g < KB; ++g) {
        const int k = 16 * g + 4 * q;
        const float4 a0 = *reinterpret_cast<const float4 *>(A + m * lda + k);
        const float4 a1 = *reinterpret_cast<const float4 *>(A + (16 + m) * lda + k);
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            if (i >= ntw) break;
            const int j = 16 * (t0 + 4 * i) + m;
            float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j < J) b = gt_ld4(W + (size_t)j * ldw, k, K, vec);
            acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, b.x, acc[i][0], 0, 0, 0);
            acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, b.x, acc[i][1], 0, 0, 0);
            acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, b.y, acc[i][0], 0, 0, 0);
            acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, b.y, acc[i][1], 0, 0, 0);
            acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, b.z, acc[i][0], 0, 0, 0);
            acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, b.z, acc[i][1], 0, 0, 0);
            acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, b.w, acc[i][0], 0, 0, 0);
            acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, b.w, acc[i][1], 0, 0, 0);
        }
    }
}

// token LayerNorm / FFN weights of one layer in LDS, zero-padded to 32 tokens x 16 hidden units
struct GtTok {
    float *lg, *lb, *w1, *b1, *w2, *b2;
};
__device__ __forceinline__ GtTok gt_tok_ptrs(float *p) {
    GtTok t;
    t.lg = p;
    t.lb = t.lg + GT_MT;
    t.w1 = t.lb + GT_MT;              // [16][32]
    t.b1 = t.w1 + GT_HTP * GT_MT;
    t.w2 = t.b1 + GT_HTP;             // [32][16]
    t.b2 = t.w2 + GT_MT * GT_HTP;
    return t;
}
__device__ __forceinline__ void gt_tok_load(const GtTok &t, const float *const *w, int N, int HT) {
    for (int i = threadIdx.x; i < GT_MT * GT_HTP; i += blockDim.x) {
        const int j = i / GT_MT, n = i % GT_MT;
        t.w1[i] = (j < HT && n < N) ? w[2][j * N + n] : 0.f;
        const int n2 = i / GT_HTP, j2 = i % GT_HTP;
        t.w2[i] = (j2 < HT && n2 < N) ? w[4][n2 * HT + j2] : 0.f;
    }
    for (int i = threadIdx.x; i < GT_MT; i += blockDim.x) {
        t.lg[i] = i < N ? w[0][i] : 0.f;
        t.lb[i] = i < N ? w[1][i] : 0.f;
        t.b2[i] = i < N ? w[5][i] : 0.f;
        if (i < GT_HTP) t.b1[i] = i < HT ? w[3][i] : 0.f;
    }
}

// images the backward emits for one (row, channel): rows of the [R C][32] / [R C][16] matrices
struct GtTokOut {
    float *Yt, *dYt, *Gt, *dOt, *Ht, *dHt;
};

__device__ __forceinline__ void gt_st_row(float *dst, const float *v, int n) {
#pragma unroll
    for (int i = 0; i < n; i += 4) *reinterpret_cast<float4 *>(dst + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
}

// Token mixing of channel c of the row image X (:289-297), one thread: y = LN_t(X[:, c]), h = drop(gelu(W1 y + b1)),
// X[:, c] += drop(W2 h + b2).  BWD: X holds the layer input, D the gradient of the mixed column; D[:, c] becomes
// the gradient of the input column, and the weight-gradient operands go to `o`.
template <bool BWD>
__device__ __forceinline__ void gt_tok(float *X, float *D, int XP, int c, int N, int HT, const GtTok &w,
                                       const uint8_t *kh, const uint8_t *ko, float scale, const GtTokOut &o) {
    float xh[GT_MT], y[GT_MT];
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < GT_MT; ++t) {
        xh[t] = t < N ? X[t * XP + c] : 0.f;
        s += xh[t];
    }
    const float mean = s / (float)N;
    float qv = 0.f;
#pragma unroll
    for (int t = 0; t < GT_MT; ++t) {
        const float d = t < N ? xh[t] - mean : 0.f;
        qv += d * d;
        xh[t] = d;
    }
    const float rstd = 1.f / sqrtf(qv / (float)N + 1e-5f);
#pragma unroll
    for (int t = 0; t < GT_MT; ++t) {
        xh[t] *= rstd;
        y[t] = xh[t] * w.lg[t] + w.lb[t];   // lg = lb = 0 past N
    }
    float hp[GT_HTP], hd[GT_HTP];
#pragma unroll
    for (int j = 0; j < GT_HTP; ++j) {
        float a = w.b1[j];
#pragma unroll
        for (int t = 0; t < GT_MT; ++t) a += w.w1[j * GT_MT + t] * y[t];
        hp[j] = a;
        hd[j] = j < HT ? gm_gelu(a) * gt_kf(kh, j, scale) : 0.f;
    }
    if (!BWD) {
#pragma unroll
        for (int t = 0; t < GT_MT; ++t) {
            float a = w.b2[t];
#pragma unroll
            for (int j = 0; j < GT_HTP; ++j) a += w.w2[t * GT_HTP + j] * hd[j];
            if (t < N) X[t * XP + c] += a * gt_kf(ko, t, scale);
        }
        return;
    }
    gt_st_row(o.Yt, y, GT_MT);
    gt_st_row(o.Ht, hd, GT_HTP);
    float dO[GT_MT];
#pragma unroll
    for (int t = 0; t < GT_MT; ++t) dO[t] = t < N ? D[t * XP + c] * gt_kf(ko, t, scale) : 0.f;
    gt_st_row(o.dOt, dO, GT_MT);
    float dh[GT_HTP];
#pragma unroll
    for (int j = 0; j < GT_HTP; ++j) {
        float a = 0.f;
#pragma unroll
        for (int t = 0; t < GT_MT; ++t) a += w.w2[t * GT_HTP + j] * dO[t];
        dh[j] = j < HT ? a * gt_kf(kh, j, scale) * gm_gelu_d(hp[j]) : 0.f;
    }
    gt_st_row(o.dHt, dh, GT_HTP);
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int t = 0; t < GT_MT; ++t) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < GT_HTP; ++j) a += w.w1[j * GT_MT + t] * dh[j];
        y[t] = a;             // d y
        dO[t] = a * xh[t];    // d LN weight operand
        const float dxh = a * w.lg[t];
        m1 += dxh;
        m2 += dxh * xh[t];
    }
    gt_st_row(o.dYt, y, GT_MT);
    gt_st_row(o.Gt, dO, GT_MT);
    m1 /= (float)N;
    m2 /= (float)N;
#pragma unroll
    for (int t = 0; t < GT_MT; ++t)
        if (t < N) D[t * XP + c] += rstd * (y[t] * w.lg[t] - m1 - xh[t] * m2);
}

// LDS plan of the forward (floats): X [32][XP] | Y [32][XP] | H [32][HP] | token weights | valid [32]
__host__ __device__ inline size_t gt_fwd_lds_floats(int C, int T) {
    const int XP = gm_r16(std::max(C, T)) + 4;
    return (size_t)2 * GT_MT * XP + (size_t)GT_MT * (GT_HCH + 4) + GT_TOKW + GT_MT;
}
// the backward: X | Y | D | DO [32][XP] each | H [32][HP] | token weights | valid, rstd [2][32]
__host__ __device__ inline size_t gt_bwd_lds_floats(int C) {
    const int XP = gm_r16(C) + 4;
    return (size_t)4 * GT_MT * XP + (size_t)GT_MT * (GT_HCH + 4) + GT_TOKW + 2 * GT_MT;
}

__global__ void __launch_bounds__(256) gt_fwd_kernel(GtArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gt_lds[];
    const int r = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int N = a.N, C = a.C, T = a.T, D = a.D, HC = a.HC, R = a.R;
    const int C16 = gm_r16(C), XP = gm_r16(max(C, T)) + 4, HP = GT_HCH + 4;
    float *X = gt_lds, *Y = X + GT_MT * XP, *H = Y + GT_MT * XP, *tokp = H + GT_MT * HP, *sval = tokp + GT_TOKW;
    const GtTok tok = gt_tok_ptrs(tokp);
    const GtWs ws = gt_ws(R, N, C, T, a.L, HC);
    const GtKeep kp = gt_keep(R, N, C, a.HT, HC);
    for (int i = tid; i < 2 * GT_MT * XP + GT_MT * HP; i += blockDim.x) gt_lds[i] = 0.f;
    if (tid < GT_MT) sval[tid] = (tid < N && a.nid[(size_t)r * N + tid] != 0) ? 1.f : 0.f;
    __syncthreads();
    const int NT = C16 / 16, ntw = (NT - wave + 3) / 4;   // this wave's output tiles: wave + 4 i, i < ntw
    const int m = lane & 15, q = lane >> 4;
    // ---- projection (:156-167): X = [E(e) | cos(dt w + b)] Wp^T + bp, the two K parts through Y in turn
    {
        gtx4 acc[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = gtx4{0.f, 0.f, 0.f, 0.f};
        const double cut = a.cut[r];
        const int ldp = C + T;
        const bool vecp = ldp % 4 == 0 && C % 4 == 0;
        for (int pass = 0; pass < 2; ++pass) {
            const int K = pass ? T : C, K16 = gm_r16(K);
            if (K <= 0) continue;
            for (int i = tid; i < GT_MT * K16; i += blockDim.x) {
                const int t = i / K16, k = i - t * K16;
                float v = 0.f;
                if (t < N && k < K) {
                    if (sval[t] != 0.f) {
                        if (pass == 0) v = a.e_feat[(size_t)a.eid[(size_t)r * N + t] * C + k];
                        else {
                            // Linear(1, d) on fp32 dt: one rounding of dt * w + b (the reference's CPU addmm)
                            const float dt = (float)(cut - a.ts[(size_t)r * N + t]);
                            v = cos_rd((float)((double)dt * (double)a.time_w[k] + (double)a.time_b[k]));
                        }
                    }
                    a.ws[ws.F + ((int64_t)r * N + t) * ws.ldK + pass * C + k] = v;
                }
                Y[t * XP + k] = v;
            }
            __syncthreads();
            gt_gemm<4>(Y, XP, K16 / 16, a.proj_w + pass * C, ldp, C, K, vecp, wave, ntw, acc);
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i >= ntw) break;
            const int n = 16 * (wave + 4 * i) + m;
            const float bv = n < C ? a.proj_b[n] : 0.f;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int t = 16 * mt + 4 * q + e;
                    if (t < N && n < C) X[t * XP + n] = acc[i][mt][e] + bv;
                }
        }
    }
    __syncthreads();
    for (int l = 0; l < a.L; ++l) {
        const float *const *w = a.lw + 14 * l;
        const uint8_t *keep = a.keep ? a.keep + (int64_t)l * kp.layer : nullptr;
        // the layer's input image, kept for the backward
        float *xl = a.ws + ws.XL + ((int64_t)l * R + r) * N * ws.ldC;
        for (int i = tid; i < N * C; i += blockDim.x) {
            const int t = i / C, c = i - t * C;
            xl[t * ws.ldC + c] = X[t * XP + c];
        }
        gt_tok_load(tok, w, N, a.HT);
        __syncthreads();
        // ---- token mixing (:289-297), one thread per channel
        if (tid < C) {
            const int64_t rc = (int64_t)r * C + tid;
            gt_tok<false>(X, nullptr, XP, tid, N, a.HT, tok, keep ? keep + kp.tok_h + rc * a.HT : nullptr,
                          keep ? keep + kp.tok_o + rc * N : nullptr, a.keep_scale, GtTokOut{});
        }
        __syncthreads();
        // ---- channel LayerNorm (:300), one wave per token, into Y (zero past N / C)
        for (int t = wave; t < GT_MT; t += 4) {
            float mean = 0.f, rstd = 0.f;
            if (t < N) {
                float s = 0.f, qq = 0.f;
                for (int c = lane; c < C; c += 64) s += X[t * XP + c];
                mean = gm_wsum(s) / (float)C;
                for (int c = lane; c < C; c += 64) {
                    const float d = X[t * XP + c] - mean;
                    qq += d * d;
                }
                rstd = 1.f / sqrtf(gm_wsum(qq) / (float)C + 1e-5f);
            }
            for (int c = lane; c < C16; c += 64)
                Y[t * XP + c] = (t < N && c < C) ? (X[t * XP + c] - mean) * rstd * w[6][c] + w[7][c] : 0.f;
        }
        __syncthreads();
        // ---- channel FFN (:302-305): hidden chunks of GT_HCH through LDS, the second GEMM accumulating in registers
        gtx4 acc2[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc2[i][0] = acc2[i][1] = gtx4{0.f, 0.f, 0.f, 0.f};
        const bool vecc = C % 4 == 0, vech = HC % 4 == 0;
        for (int h0 = 0; h0 < HC; h0 += GT_HCH) {
            const int nh = min(GT_HCH, HC - h0), tiles = gm_r16(nh) / 16, nw1 = (tiles - wave + 3) / 4;
            gtx4 acc1[2][2];
#pragma unroll
            for (int i = 0; i < 2; ++i) acc1[i][0] = acc1[i][1] = gtx4{0.f, 0.f, 0.f, 0.f};
            gt_gemm<2>(Y, XP, C16 / 16, w[8] + (size_t)h0 * C, C, nh, C, vecc, wave, nw1, acc1);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (i >= nw1) break;
                const int jj = 16 * (wave + 4 * i) + m, n = h0 + jj;
                const float bv = n < HC ? w[9][n] : 0.f;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int t = 16 * mt + 4 * q + e;
                        float v = 0.f;
                        if (t < N && n < HC)
                            v = gm_gelu(acc1[i][mt][e] + bv) *
                                gt_kf(keep, kp.ch_h + ((int64_t)r * N + t) * HC + n, a.keep_scale);
                        H[t * HP + jj] = v;
                    }
            }
            __syncthreads();
            gt_gemm<4>(H, HP, tiles, w[10] + h0, HC, C, nh, vech, wave, ntw, acc2);
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i >= ntw) break;
            const int n = 16 * (wave + 4 * i) + m;
            const float bv = n < C ? w[11][n] : 0.f;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int t = 16 * mt + 4 * q + e;
                    if (t < N && n < C)
                        X[t * XP + n] += (acc2[i][mt][e] + bv) *
                                         gt_kf(keep, kp.ch_o + ((int64_t)r * N + t) * C + n, a.keep_scale);
                }
        }
        __syncthreads();
    }
    // ---- masked mean over the tokens (:176-178) and the neighbour-feature mean (:181-189)
    for (int c = tid; c < C; c += blockDim.x) {
        float s = 0.f;
        for (int t = 0; t < N; ++t) s += X[t * XP + c] * sval[t];
        a.x_mean[(size_t)r * C + c] = s / (float)N;
    }
    float nvalid = 0.f;
    for (int t = 0; t < N; ++t) nvalid += sval[t];
    for (int d = tid; d < D; d += blockDim.x) {
        float s = 0.f;
        for (int t = 0; t < N; ++t) {
            // softmax(valid ? 1 : -1e10): 1 / n_valid on valid neighbours, 1 / N everywhere when none is valid
            const float sc = nvalid > 0.f ? sval[t] / nvalid : 1.f / (float)N;
            s += a.n_feat[(size_t)a.nid[(size_t)r * N + t] * D + d] * sc;
        }
        a.node_out[(size_t)r * D + d] = s / (float)N + a.n_feat[(size_t)a.node[r] * D + d];
    }
}

// Layer l's backward for row r = blockIdx.x.  d_x_mean feeds the last layer; d X_l is handed on through ws.DX.
__global__ void __launch_bounds__(256) gt_bwd_layer_kernel(GtArgs a, const float *__restrict__ d_x_mean, int l) {
    extern __shared__ __attribute__((aligned(16))) float gt_lds[];
    const int r = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int N = a.N, C = a.C, HC = a.HC, R = a.R;
    const int C16 = gm_r16(C), XP = C16 + 4, HP = GT_HCH + 4;
    float *X = gt_lds, *Y = X + GT_MT * XP, *Dm = Y + GT_MT * XP, *DO = Dm + GT_MT * XP, *H = DO + GT_MT * XP;
    float *tokp = H + GT_MT * HP, *sval = tokp + GT_TOKW, *trstd = sval + GT_MT;
    const GtTok tok = gt_tok_ptrs(tokp);
    const GtWs ws = gt_ws(R, N, C, a.T, a.L, HC);
    const GtKeep kp = gt_keep(R, N, C, a.HT, HC);
    const float *const *w = a.lw + 14 * l;
    const uint8_t *keep = a.keep ? a.keep + (int64_t)l * kp.layer : nullptr;
    const int64_t rn0 = (int64_t)r * N;
    const float *xl = a.ws + ws.XL + ((int64_t)l * R + r) * N * ws.ldC;
    float *dx = a.ws + ws.DX + rn0 * ws.ldC;
    if (tid < GT_MT) sval[tid] = (tid < N && a.nid[(size_t)r * N + tid] != 0) ? 1.f : 0.f;
    for (int i = tid; i < GT_MT * HP; i += blockDim.x) H[i] = 0.f;
    __syncthreads();
    // ---- D = d (layer output), X = the layer's input (zero past N / C)
    for (int i = tid; i < GT_MT * C16; i += blockDim.x) {
        const int t = i / C16, c = i - t * C16;
        const bool in = t < N && c < C;
        float d = 0.f;
        if (in) d = l == a.L - 1 ? d_x_mean[(size_t)r * C + c] * sval[t] / (float)N : dx[t * ws.ldC + c];
        Dm[t * XP + c] = d;
        X[t * XP + c] = in ? xl[t * ws.ldC + c] : 0.f;
    }
    gt_tok_load(tok, w, N, a.HT);
    __syncthreads();
    const int64_t rc = (int64_t)r * C + tid;
    const uint8_t *kth = keep ? keep + kp.tok_h + rc * a.HT : nullptr, *kto = keep ? keep + kp.tok_o + rc * N : nullptr;
    if (tid < C) gt_tok<false>(X, nullptr, XP, tid, N, a.HT, tok, kth, kto, a.keep_scale, GtTokOut{});
    __syncthreads();
    // ---- channel LayerNorm recomputed: X <- xhat, Y <- LN output; DO = d (FFN output before its dropout)
    for (int t = wave; t < GT_MT; t += 4) {
        float mean = 0.f, rstd = 0.f;
        if (t < N) {
            float s = 0.f, qq = 0.f;
            for (int c = lane; c < C; c += 64) s += X[t * XP + c];
            mean = gm_wsum(s) / (float)C;
            for (int c = lane; c < C; c += 64) {
                const float d = X[t * XP + c] - mean;
                qq += d * d;
            }
            rstd = 1.f / sqrtf(gm_wsum(qq) / (float)C + 1e-5f);
        }
        if (lane == 0) trstd[t] = rstd;
        for (int c = lane; c < C16; c += 64) {
            const bool in = t < N && c < C;
            const float xh = in ? (X[t * XP + c] - mean) * rstd : 0.f;
            const float y = in ? xh * w[6][c] + w[7][c] : 0.f;
            const float dOv = in ? Dm[t * XP + c] * gt_kf(keep, kp.ch_o + (rn0 + t) * C + c, a.keep_scale) : 0.f;
            X[t * XP + c] = xh;
            Y[t * XP + c] = y;
            DO[t * XP + c] = dOv;
            if (in) {
                a.ws[ws.Yc + (rn0 + t) * ws.ldC + c] = y;
                a.ws[ws.dOc + (rn0 + t) * ws.ldC + c] = dOv;
            }
        }
    }
    __syncthreads();
    // ---- channel FFN: per hidden chunk, the pre-activations again (Y W0^T) and d hidden (DO W3) on the same
    // output tiles, so both are in the same registers; d pre-activation through LDS into d Y += dH W0
    const int NT = C16 / 16, ntw = (NT - wave + 3) / 4, m = lane & 15, q = lane >> 4;
    const bool vecc = C % 4 == 0, vech = HC % 4 == 0;
    gtx4 accy[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) accy[i][0] = accy[i][1] = gtx4{0.f, 0.f, 0.f, 0.f};
    for (int h0 = 0; h0 < HC; h0 += GT_HCH) {
        const int nh = min(GT_HCH, HC - h0), tiles = gm_r16(nh) / 16, nw1 = (tiles - wave + 3) / 4;
        gtx4 acc1[2][2], accd[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i) acc1[i][0] = acc1[i][1] = accd[i][0] = accd[i][1] = gtx4{0.f, 0.f, 0.f, 0.f};
        gt_gemm<2>(Y, XP, C16 / 16, w[8] + (size_t)h0 * C, C, nh, C, vecc, wave, nw1, acc1);
        gt_gemm<2>(DO, XP, C16 / 16, w[12] + (size_t)h0 * C, C, nh, C, vecc, wave, nw1, accd);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (i >= nw1) break;
            const int jj = 16 * (wave + 4 * i) + m, n = h0 + jj;
            const float bv = n < HC ? w[9][n] : 0.f;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int t = 16 * mt + 4 * q + e;
                    float dh = 0.f;
                    if (t < N && n < HC) {
                        const float hp = acc1[i][mt][e] + bv;
                        const float kf = gt_kf(keep, kp.ch_h + (rn0 + t) * HC + n, a.keep_scale);
                        dh = accd[i][mt][e] * kf * gm_gelu_d(hp);
                        a.ws[ws.Hc + (rn0 + t) * ws.ldH + n] = gm_gelu(hp) * kf;
                        a.ws[ws.dHc + (rn0 + t) * ws.ldH + n] = dh;
                    }
                    H[t * HP + jj] = dh;
                }
        }
        __syncthreads();
        gt_gemm<4>(H, HP, tiles, w[13] + h0, HC, C, nh, vech, wave, ntw, accy);
        __syncthreads();
    }
    // d Y over DO (every wave is past its last read of it)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i >= ntw) break;
        const int n = 16 * (wave + 4 * i) + m;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int t = 16 * mt + 4 * q + e;
                if (t < N && n < C) DO[t * XP + n] = accy[i][mt][e];
            }
    }
    __syncthreads();
    // ---- channel LayerNorm backward, one wave per token: D += d (LN input)
    for (int t = wave; t < N; t += 4) {
        float s1 = 0.f, s2 = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float dxh = DO[t * XP + c] * w[6][c];
            s1 += dxh;
            s2 += dxh * X[t * XP + c];
        }
        const float m1 = gm_wsum(s1) / (float)C, m2 = gm_wsum(s2) / (float)C, rstd = trstd[t];
        for (int c = lane; c < C; c += 64) {
            const float dy = DO[t * XP + c], xh = X[t * XP + c];
            Dm[t * XP + c] += rstd * (dy * w[6][c] - m1 - xh * m2);
            a.ws[ws.dYc + (rn0 + t) * ws.ldC + c] = dy;
            a.ws[ws.Gc + (rn0 + t) * ws.ldC + c] = dy * xh;
        }
    }
    __syncthreads();
    // ---- token mixing backward on the layer's input again
    for (int i = tid; i < N * C; i += blockDim.x) {
        const int t = i / C, c = i - t * C;
        X[t * XP + c] = xl[t * ws.ldC + c];
    }
    __syncthreads();
    if (tid < C) {
        GtTokOut o;
        o.Yt = a.ws + ws.Yt + rc * GT_MT;
        o.dYt = a.ws + ws.dYt + rc * GT_MT;
        o.Gt = a.ws + ws.Gt + rc * GT_MT;
        o.dOt = a.ws + ws.dOt + rc * GT_MT;
        o.Ht = a.ws + ws.Ht + rc * GT_HTP;
        o.dHt = a.ws + ws.dHt + rc * GT_HTP;
        gt_tok<true>(X, Dm, XP, tid, N, a.HT, tok, kth, kto, a.keep_scale, o);
    }
    __syncthreads();
    for (int i = tid; i < N * C; i += blockDim.x) {
        const int t = i / C, c = i - t * C;
        dx[t * ws.ldC + c] = Dm[t * XP + c];
    }
}

static int gt_check(const tm_gm_embed_args &q, const char *what) {
    if (q.R < 0 || q.N <= 0 || q.C <= 0 || q.T < 0 || q.D <= 0 || q.L < 0 || q.HT < 0 || q.HC <= 0)
        return fail(TM_E_ARG, std::string(what) + ": bad dimensions");
    if (q.ew || q.edge_attr)
        return fail(TM_E_UNSUPPORTED, std::string(what) + ": explanation weights / edge_attr are not part of the "
                                                          "base model's training step");
    if (!tm_gm_train_ok(q.N, q.C, q.T, q.L, q.HT, q.HC))
        return fail(TM_E_UNSUPPORTED, std::string(what) + ": needs num_tokens <= 32, 1 <= token hidden <= 16, 1 to 4 "
                                                          "layers, channels and time dim <= 256");
    return TM_OK;
}

static GtArgs gt_args(const tm_gm_embed_args &q, const uint8_t *keep, float keep_scale, void *workspace) {
    GtArgs a{};
    a.R = q.R; a.N = q.N; a.C = q.C; a.T = q.T; a.D = q.D; a.L = q.L; a.HT = q.HT; a.HC = q.HC;
    a.node = q.node; a.nid = q.nid; a.eid = q.eid; a.cut = q.cut; a.ts = q.ts;
    a.n_feat = q.n_feat; a.e_feat = q.e_feat; a.time_w = q.time_w; a.time_b = q.time_b;
    a.proj_w = q.proj_w; a.proj_b = q.proj_b;
    a.lw = q.layer_table;
    a.keep = keep;
    a.keep_scale = keep_scale;
    a.x_mean = q.x_mean;
    a.node_out = q.node_out;
    a.ws = reinterpret_cast<float *>(workspace);
    return a;
}

}  // namespace tmk

using namespace tmk;

extern "C" int tm_gm_train_ok(int32_t N, int32_t C, int32_t T, int32_t L, int32_t HT, int32_t HC) {
    return N > 0 && N <= GT_MT && HT >= 1 && HT <= GT_HTP && L >= 1 && L <= GT_MAXL && C > 0 && C <= 256 && T >= 0 &&
           T <= 256 && HC > 0 && sizeof(float) * gt_bwd_lds_floats(C) <= 160 * 1024 &&
           sizeof(float) * gt_fwd_lds_floats(C, T) <= 160 * 1024;
}

extern "C" int64_t tm_gm_train_workspace_bytes(int64_t R, int32_t N, int32_t C, int32_t T, int32_t L, int32_t HT,
                                               int32_t HC) {
    if (R < 0 || !tm_gm_train_ok(N, C, T, L, HT, HC)) return -1;
    return (int64_t)sizeof(float) * gt_ws(std::max<int64_t>(R, 1), N, C, T, L, HC).total;
}

extern "C" int tm_gm_train_fwd(const tm_gm_embed_args *p, const uint8_t *keep, float keep_scale, void *workspace,
                               void *stream) {
    if (!p) return fail(TM_E_ARG, "tm_gm_train_fwd: NULL arguments");
    const tm_gm_embed_args &q = *p;
    int rc = gt_check(q, "tm_gm_train_fwd");
    if (rc != TM_OK) return rc;
    if (q.R == 0) return TM_OK;
    if (!q.node || !q.nid || !q.eid || !q.cut || !q.ts || !q.n_feat || !q.e_feat || (q.T && (!q.time_w || !q.time_b)) ||
        !q.proj_w || !q.proj_b || !q.x_mean || !q.node_out || !workspace || !q.layer_table)
        return fail(TM_E_ARG, "tm_gm_train_fwd: NULL pointer");
    const GtArgs a = gt_args(q, keep, keep_scale, workspace);
    const size_t lds = sizeof(float) * gt_fwd_lds_floats(q.C, q.T);
    hipEvent_t pe = prof_begin((hipStream_t)stream);
    TM_HIP(hipFuncSetAttribute((const void *)gt_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    gt_fwd_kernel<<<q.R, 256, lds, (hipStream_t)stream>>>(a);
    TM_CHECK_LAUNCH();
    prof_end("gt_fwd_kernel", (hipStream_t)stream, pe);
    return TM_OK;
}

extern "C" int tm_gm_train_bwd(const tm_gm_embed_args *p, const uint8_t *keep, float keep_scale, void *workspace,
                               const float *d_x_mean, float *const *grads, void *stream) {
    if (!p || !grads) return fail(TM_E_ARG, "tm_gm_train_bwd: NULL arguments");
    const tm_gm_embed_args &q = *p;
    int rc = gt_check(q, "tm_gm_train_bwd");
    if (rc != TM_OK) return rc;
    for (int i = 0; i < 2 + 12 * q.L; ++i)
        if (!grads[i]) return fail(TM_E_ARG, "tm_gm_train_bwd: NULL gradient pointer");
    hipStream_t s = (hipStream_t)stream;
    const int N = q.N, C = q.C, HT = q.HT, HC = q.HC, K = q.C + q.T;
    if (q.R == 0) {   // no rows: every gradient is zero
        TM_HIP(hipMemsetAsync(grads[0], 0, sizeof(float) * C * K, s));
        TM_HIP(hipMemsetAsync(grads[1], 0, sizeof(float) * C, s));
        for (int l = 0; l < q.L; ++l) {
            const int64_t n[12] = {N, N, (int64_t)HT * N, HT, (int64_t)N * HT, N, C, C, (int64_t)HC * C, HC, (int64_t)C * HC, C};
            for (int i = 0; i < 12; ++i) TM_HIP(hipMemsetAsync(grads[2 + 12 * l + i], 0, sizeof(float) * n[i], s));
        }
        return TM_OK;
    }
    if (!q.nid || !d_x_mean || !workspace || !q.layer_table)
        return fail(TM_E_ARG, "tm_gm_train_bwd: NULL pointer");
    const GtArgs a = gt_args(q, keep, keep_scale, workspace);
    const GtWs ws = gt_ws(q.R, N, C, q.T, q.L, HC);
    float *W = a.ws;
    const int RN = q.R * N, RC = q.R * C;
    const size_t lds = sizeof(float) * gt_bwd_lds_floats(C);
    TM_HIP(hipFuncSetAttribute((const void *)gt_bwd_layer_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (int l = q.L - 1; l >= 0; --l) {
        hipEvent_t pe = prof_begin(s);
        gt_bwd_layer_kernel<<<q.R, 256, lds, s>>>(a, d_x_mean, l);
        TM_CHECK_LAUNCH();
        prof_end("gt_bwd_layer_kernel", s, pe);
        float *const *g = grads + 2 + 12 * l;
        float *dm = W + ws.dummy;
        const tm_wgrad_job jobs[8] = {
            {W + ws.dHt, W + ws.Yt, GT_HTP, GT_MT, HT, N, RC},        // token ffn.0
            {W + ws.dOt, W + ws.Ht, GT_MT, GT_HTP, N, HT, RC},        // token ffn.3
            {W + ws.Gt, W + ws.Gt, GT_MT, GT_MT, N, 1, RC},           // token_norm weight (column sums)
            {W + ws.dYt, W + ws.dYt, GT_MT, GT_MT, N, 1, RC},         // token_norm bias
            {W + ws.dHc, W + ws.Yc, ws.ldH, ws.ldC, HC, C, RN},       // channel ffn.0
            {W + ws.dOc, W + ws.Hc, ws.ldC, ws.ldH, C, HC, RN},       // channel ffn.3
            {W + ws.Gc, W + ws.Gc, ws.ldC, ws.ldC, C, 1, RN},         // channel_norm weight
            {W + ws.dYc, W + ws.dYc, ws.ldC, ws.ldC, C, 1, RN},       // channel_norm bias
        };
        const tm_wgrad_target tgts[8] = {{g[2], g[3], 0, 1}, {g[4], g[5], 1, 1}, {dm, g[0], 2, 1},
                                         {dm + 256, g[1], 3, 1}, {g[8], g[9], 4, 1}, {g[10], g[11], 5, 1},
                                         {dm + 512, g[6], 6, 1}, {dm + 768, g[7], 7, 1}};
        rc = tm_wgrad(jobs, 8, tgts, 8, stream);
        if (rc != TM_OK) return rc;
    }
    // projection: dW = dX_0^T F, db = column sums of dX_0
    const tm_wgrad_job pj = {W + ws.DX, W + ws.F, ws.ldC, ws.ldK, C, K, RN};
    const tm_wgrad_target pt = {grads[0], grads[1], 0, 1};
    return tm_wgrad(&pj, 1, &pt, 1, stream);
}
