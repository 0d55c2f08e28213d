// Skinny weight-streaming GEMM for the decode step: out[M, N] = x[M, K] . W[N, K]^T with
// M = CFG-doubled batch (1..256), i.e. HBM/latency-bound on the weight stream.
//
// Replaces the nn.Linear calls of the reference decode step
// (autoregressive/models/gpt.py:161-163 w1/w3/w2, :199-200 wqkv/wo, :287 output) and fuses
// what the reference does around them:
//   NORM prologue : RMSNorm of the input rows (gpt.py:143-148) applied to the B operand on the fly;
//                   the row sums of squares arrive as partials written by the producer kernel
//   EPI_QKV    : wqkv + apply_rotary_emb(q, k) + KVCache.update   (gpt.py:214-226, 177-185, 420-430)
//   EPI_RES    : wo / w2 + residual add (gpt.py:238-240, 255-256) [+ partial row sums of squares of
//                the new residual stream for the next RMSNorm]
//   EPI_SWIGLU : silu(w1 x) * w3 x on a row-interleaved w1||w3    (gpt.py:167)
//   EPI_ROWS   : row-major output (lm_head logits, gpt.py:367-368)
//   EPI_PACKED / EPI_GELU : plain / gelu(tanh) packed output (CaptionEmbedder MLP, gpt.py:118-131)
//
// Design (MI355X-first): both operands live in HBM in MFMA-fragment order, so
// every wave-level load is one fully coalesced 1 KiB `global_load_dwordx4`, straight into the
// VGPRs that feed `v_mfma_f32_16x16x32_bf16` (or 4 x `v_mfma_f32_16x16x4_f32` in fp32 mode):
// no LDS staging, no barriers in the main loop.  A workgroup owns NT 16-row tiles of N for all
// M rows; its KW waves split K between them, each keeps DEPTH k-chunks of loads in flight
// (register ring, static indices) and they combine through LDS in a fixed order (deterministic,
// no atomics).  Weight loads use the default cache policy (lanes a few layers apart share the stream in the
// memory-side cache: 69.4 vs 65.7 img/s against non-temporal loads with 3 lanes, no difference with one).  Everything an epilogue
// needs from memory (residual tile, RoPE angles) is requested before the main loop.
#include <cstdlib>
#include <type_traits>

#include "lgen_common.h"
#include "../../include/lgen.h"

#include "gemm_epilogue.h"

// VGPR budget: DEPTH register stages of operands + accumulators + prefetched epilogue operands
// (+ RMSNorm scales / weights / temporaries).  DEPTH shrinks for the big tile shapes so that nothing
// spills; <= 120 registers -> 16 waves (1024 threads) may share a CU's SIMDs, else 8 waves.
template <int MT, int NT, bool NORM, int EPI>
constexpr int gemm_fixed_regs() {
    return NT * MT * 4 + (epi_has_aux<EPI>() ? NT * MT * 4 : 0) + (NORM ? 44 : 0) + (epi_qkv(EPI) ? 16 : 0) + 36;
}
template <int MT, int NT, bool NORM, int EPI>
constexpr int gemm_depth() {
    constexpr int per_stage = (NT + MT + (NORM ? 1 : 0)) * 4;
    constexpr int d = (200 - gemm_fixed_regs<MT, NT, NORM, EPI>()) / per_stage;
    return d < 2 ? 2 : (d > 6 ? 6 : d);
}
template <int MT, int NT, bool NORM, int EPI>
constexpr int gemm_max_threads() {
    return (gemm_depth<MT, NT, NORM, EPI>() * (NT + MT + (NORM ? 1 : 0)) * 4 + gemm_fixed_regs<MT, NT, NORM, EPI>() > 124) ? 512 : 1024;
}

template <typename D, int MT, int NT, int EPI, bool NORM, int DEPTH>
__global__ __launch_bounds__((gemm_max_threads<MT, NT, NORM, EPI>())) void gemm_kernel(GemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float4 red[];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int KW = blockDim.x >> 6;
    const int nt0 = blockIdx.x * NT;
    const int mt0 = blockIdx.y * MT;
    const int k0 = (int)(((long)a.KCH * w) / KW), k1 = (int)(((long)a.KCH * (w + 1)) / KW);
    int posr[MT];
    load_row_pos<MT, EPI>(a, mt0, lane, posr);

    const uint4* wbase = a.wp + ((size_t)nt0 * a.KCH) * 64 + lane;
    const uint4* xbase = a.xp + (size_t)mt0 * 64 + lane;
    const size_t wstride = (size_t)a.KCH * 64;
    const size_t xstride = (size_t)a.MTs * 64;

    uint4 A[DEPTH][NT], B[DEPTH][MT], WN[DEPTH];
#define LGEN_LOAD(s, kk)                                                                                  \
    {                                                                                                     \
        _Pragma("unroll") for (int j = 0; j < NT; ++j) A[s][j] = ldg_w(wbase + j * wstride + (size_t)(kk) * 64); \
        _Pragma("unroll") for (int i = 0; i < MT; ++i) B[s][i] = xbase[(size_t)(kk) * xstride + i * 64];  \
        if constexpr (NORM) WN[s] = a.nw[(size_t)(kk) * 4 + (lane >> 4)];                                \
    }
    // 1. fill the ring
#pragma unroll
    for (int s = 0; s < DEPTH; ++s)
        if (k0 + s < k1) LGEN_LOAD(s, k0 + s);

    // 2. request what the epilogue will need (this wave's units)
    uint4 aux[gemm_units<MT, NT, EPI>()];
    gemm_aux_prefetch<D, MT, NT, EPI>(a, aux, w, KW, lane, nt0, mt0, posr);

    // 3. RMSNorm row scales from the producer's partial sums of squares (fixed order)
    float ri[MT];
    if constexpr (NORM) {
        float ssum[MT];
        ssq_rows_now<MT>(a.ssq_in, a.parts, mt0, lane, ssum);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            float s = ssum[i];
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            ri[i] = 1.0f / sqrtf(s * a.inv_k + a.eps);
        }
    }

    f32x4_t acc[NT][MT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[j][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

#define LGEN_MMA(s)                                                                                       \
    {                                                                                                     \
        _Pragma("unroll") for (int i = 0; i < MT; ++i) {                                                  \
            uint4 b_ = B[s][i];                                                                           \
            if constexpr (NORM) b_ = D::norm_chunk(b_, ri[i], WN[s]);                                     \
            _Pragma("unroll") for (int j = 0; j < NT; ++j) acc[j][i] = D::mma(A[s][j], b_, acc[j][i]);    \
        }                                                                                                 \
    }
    // 4. main loop: consume stage s, refill it DEPTH chunks ahead
    int k = k0;
    while (k + 2 * DEPTH <= k1) {
#pragma unroll
        for (int s = 0; s < DEPTH; ++s) {
            LGEN_MMA(s);
            LGEN_LOAD(s, k + s + DEPTH);
        }
        k += DEPTH;
    }
#pragma unroll
    for (int s = 0; s < DEPTH; ++s) {
        if (k + s < k1) {
            LGEN_MMA(s);
            if (k + s + DEPTH < k1) LGEN_LOAD(s, k + s + DEPTH);
        }
    }
    k += DEPTH;
#pragma unroll
    for (int s = 0; s < DEPTH; ++s)
        if (k + s < k1) LGEN_MMA(s);
#undef LGEN_LOAD
#undef LGEN_MMA

    // 5. cross-wave K reduction + fused epilogue (gemm_epilogue.h)
    gemm_reduce_epilogue<D, MT, NT, EPI>(a, acc, red, w, KW, lane, nt0, mt0, posr, aux);
}

// ring-buffer shapes whose operand set does not fit 256 VGPRs (they would spill; csrc/gemm_skinny.usage): refused, not compiled
template <int MT, int NT, int EPI, bool NORM>
constexpr bool gemm_spills() { return NORM && (MT == 8 || (MT == 4 && NT == 4 && epi_qkv(EPI))); }

// ---- steady-state form for wide models (round 3) ---------------------------------------------------------------------
// Same operation, same wave partition and the same chunk order per wave as gemm_kernel<..., NORM = false> -- bit-identical
// results -- for K ranges that are long and uniform: every wave owns KCH / KW chunks (exact) and at least 2 * DEPTH of them
// (d = 3200, F = 8704: GPT-3B; F = 4096: GPT-XXL's w2).  What changes is what the compiler can prove about the request queue.
// In gemm_kernel the ring is filled under `if (k0 + s < k1)` and the loop may run zero times; with a conditional load in front
// of the loop the number of requests YOUNGER than a stage's loads is unknown at the loop head, so the head waits for
// vmcnt(0) -- all refills of the previous round -- and the scheduler then gathers the MFMAs of all stages behind that one
// wait: load-all / wait-all, the steady state measured in round 2 (ISA: s_waitcnt vmcnt(3) .. vmcnt(0) at the loop head,
// 200-340 TFLOP/s on GPT-3B's GEMMs).  Here the epilogue's operands are requested FIRST (older requests do not disturb the
// count), the ring fill is unconditional, the loop is do-while, and a sched_barrier after each stage keeps the stage order, so
// the waits become vmcnt((DEPTH - 1) * loads per stage): DEPTH - 1 stages stay in flight under the MFMAs of the oldest.
template <typename D, int MT, int NT, int EPI, int DEPTH>
__global__ __launch_bounds__((gemm_max_threads<MT, NT, false, EPI>())) void gemm_steady_kernel(GemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float4 red[];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int KW = blockDim.x >> 6;
    const int nt0 = blockIdx.x * NT;
    const int mt0 = blockIdx.y * MT;
    const int cpw = a.KCH / KW;  // exact, >= 2 * DEPTH (launcher)
    const int k0 = w * cpw, k1 = k0 + cpw;
    int posr[MT];
    load_row_pos<MT, EPI>(a, mt0, lane, posr);

    const uint4* wbase = a.wp + ((size_t)nt0 * a.KCH) * 64 + lane;
    const uint4* xbase = a.xp + (size_t)mt0 * 64 + lane;
    const size_t wstride = (size_t)a.KCH * 64;
    const size_t xstride = (size_t)a.MTs * 64;

    // the epilogue's operands first
    uint4 aux[gemm_units<MT, NT, EPI>()];
    gemm_aux_prefetch<D, MT, NT, EPI>(a, aux, w, KW, lane, nt0, mt0, posr);
    uint4 A[DEPTH][NT], B[DEPTH][MT];
#define LGEN_LOAD(s, kk)                                                                                  \
    {                                                                                                     \
        _Pragma("unroll") for (int j = 0; j < NT; ++j) A[s][j] = ldg_w(wbase + j * wstride + (size_t)(kk) * 64); \
        _Pragma("unroll") for (int i = 0; i < MT; ++i) B[s][i] = xbase[(size_t)(kk) * xstride + i * 64];  \
    }
#define LGEN_MMA(s)                                                                                       \
    {                                                                                                     \
        _Pragma("unroll") for (int i = 0; i < MT; ++i)                                                    \
            _Pragma("unroll") for (int j = 0; j < NT; ++j) acc[j][i] = D::mma(A[s][j], B[s][i], acc[j][i]); \
    }
#pragma unroll
    for (int s = 0; s < DEPTH; ++s) LGEN_LOAD(s, k0 + s);

    f32x4_t acc[NT][MT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[j][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    int k = k0;
    do {
#pragma unroll
        for (int s = 0; s < DEPTH; ++s) {
            LGEN_MMA(s);
            LGEN_LOAD(s, k + s + DEPTH);
            __builtin_amdgcn_sched_barrier(0);
        }
        k += DEPTH;
    } while (k + 2 * DEPTH <= k1);
#pragma unroll
    for (int s = 0; s < DEPTH; ++s) {
        if (k + s < k1) {
            LGEN_MMA(s);
            if (k + s + DEPTH < k1) LGEN_LOAD(s, k + s + DEPTH);
        }
    }
    k += DEPTH;
#pragma unroll
    for (int s = 0; s < DEPTH; ++s)
        if (k + s < k1) LGEN_MMA(s);
#undef LGEN_LOAD
#undef LGEN_MMA

    gemm_reduce_epilogue<D, MT, NT, EPI>(a, acc, red, w, KW, lane, nt0, mt0, posr, aux);
}

// tile shapes with a steady-state instantiation: the ones the host heuristics can pick for wide models at 128 / 256 rows
template <typename D, int MT, int NT, int EPI, bool NORM>
constexpr bool gemm_has_steady() {
    if (!std::is_same<D, BF16>::value || NORM) return false;
    return (EPI == EPI_RES || EPI == EPI_SWIGLU || epi_qkv(EPI) || EPI == EPI_ROWS) &&
           ((MT == 4 && (NT == 1 || NT == 2 || NT == 4)) || (MT == 2 && (NT == 2 || NT == 4)) || (MT == 8 && (NT == 1 || NT == 2)));
}

// LGEN_GEMM_STEADY=0 keeps the generic form (the parity test compares the two; read at launch = capture time)
static bool steady_enabled() {
    const char* e = getenv("LGEN_GEMM_STEADY");
    return !(e && e[0] == '0');
}


template <typename D, int MT, int NT, int EPI, bool NORM>
static int launch(const GemmArgs& a, int kw, hipStream_t st) {
    if constexpr (gemm_spills<MT, NT, EPI, NORM>()) {
        return LGEN_ERR_UNSUPPORTED;
    } else {
    constexpr int DEPTH = gemm_depth<MT, NT, NORM, EPI>();
    dim3 grid((a.N / 16) / NT, a.MTs / MT);
    size_t lds = kw > 1 ? (size_t)kw * NT * MT * 64 * sizeof(float4) : 0;
    if (lds > 160 * 1024 || kw * 64 > gemm_max_threads<MT, NT, NORM, EPI>()) return LGEN_ERR_BAD_ARG;
    if constexpr (gemm_has_steady<D, MT, NT, EPI, NORM>()) {
        if (a.KCH % kw == 0 && a.KCH / kw >= 2 * DEPTH && steady_enabled()) {
            if (lds > 64 * 1024) {
                hipError_t e = hipFuncSetAttribute((const void*)gemm_steady_kernel<D, MT, NT, EPI, DEPTH>,
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                if (e != hipSuccess) return (int)e;
            }
            hipLaunchKernelGGL((gemm_steady_kernel<D, MT, NT, EPI, DEPTH>), grid, dim3(64 * kw), lds, st, a);
            LGEN_CHECK_LAUNCH();
            return 0;
        }
    }
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)gemm_kernel<D, MT, NT, EPI, NORM, DEPTH>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((gemm_kernel<D, MT, NT, EPI, NORM, DEPTH>), grid, dim3(64 * kw), lds, st, a);
    LGEN_CHECK_LAUNCH();
    return 0;
    }
}

// the largest K-splitting wave count a (mt, nt) tile shape admits (register budget), for the host heuristics
template <int EPI, bool NORM>
static int max_kw_of(int mt, int nt) {
#define LGEN_CASE(MT_, NT_) if (mt == MT_ && nt == NT_) return gemm_spills<MT_, NT_, EPI, NORM>() ? 0 : gemm_max_threads<MT_, NT_, NORM, EPI>() / 64;
    LGEN_CASE(1, 1) LGEN_CASE(1, 2) LGEN_CASE(1, 4)
    LGEN_CASE(2, 1) LGEN_CASE(2, 2) LGEN_CASE(2, 4)
    LGEN_CASE(4, 1) LGEN_CASE(4, 2) LGEN_CASE(4, 4)
    LGEN_CASE(8, 1) LGEN_CASE(8, 2)
#undef LGEN_CASE
    return 0;
}

template <typename D, int EPI, bool NORM>
static int dispatch(const GemmArgs& a, int mt, int nt, int kw, hipStream_t st) {
    if ((a.N / 16) % nt != 0 || a.MTs % mt != 0 || kw < 1 || kw > 16) return LGEN_ERR_BAD_ARG;
    if (EPI == EPI_SWIGLU && (nt & 1)) return LGEN_ERR_BAD_ARG;
#define LGEN_CASE(MT_, NT_) if (mt == MT_ && nt == NT_) return launch<D, MT_, NT_, EPI, NORM>(a, kw, st);
    LGEN_CASE(1, 1) LGEN_CASE(1, 2) LGEN_CASE(1, 4)
    LGEN_CASE(2, 1) LGEN_CASE(2, 2) LGEN_CASE(2, 4)
    LGEN_CASE(4, 1) LGEN_CASE(4, 2) LGEN_CASE(4, 4)
    LGEN_CASE(8, 1) LGEN_CASE(8, 2)
#undef LGEN_CASE
    return LGEN_ERR_BAD_ARG;
}

template <int EPI, bool NORM>
static int dispatch_dt(const GemmArgs& a, int dtype, int mt, int nt, int kw, hipStream_t st) {
    if constexpr (EPI == EPI_QKV8) {   // the fp8 KV append exists for bf16 storage alone
        return dtype == LGEN_BF16 ? dispatch<BF16, EPI, NORM>(a, mt, nt, kw, st) : LGEN_ERR_UNSUPPORTED;
    } else {
        return lgen_dispatch_dtype(dtype, [&](auto tag) { return dispatch<decltype(tag), EPI, NORM>(a, mt, nt, kw, st); });
    }
}

// RMSNorm-prologue variants exist for the three consumers of a normalised residual stream
template <int EPI>
static int dispatch_norm(const GemmArgs& a, int dtype, int mt, int nt, int kw, hipStream_t st) {
    if (a.nw) {
        if constexpr (epi_qkv(EPI) || EPI == EPI_SWIGLU || EPI == EPI_ROWS) {
            if (!a.ssq_in || a.parts < 1) return LGEN_ERR_BAD_ARG;
            const int rc = lgen_gemm_normpre_try(a, EPI, dtype, mt, nt, kw, st);
            if (rc != LGEN_ERR_UNSUPPORTED) return rc;
            return dispatch_dt<EPI, true>(a, dtype, mt, nt, kw, st);
        } else {
            return LGEN_ERR_UNSUPPORTED;
        }
    }
    return dispatch_dt<EPI, false>(a, dtype, mt, nt, kw, st);
}

extern "C" int lgen_gemm_max_kw(int epilogue_kind, int fused_norm, int mt, int nt) {
    switch (epilogue_kind) {
        case LGEN_EPI_ROWS: return fused_norm ? max_kw_of<EPI_ROWS, true>(mt, nt) : max_kw_of<EPI_ROWS, false>(mt, nt);
        case LGEN_EPI_PACKED: return max_kw_of<EPI_PACKED, false>(mt, nt);
        case LGEN_EPI_GELU: return max_kw_of<EPI_GELU, false>(mt, nt);
        case LGEN_EPI_RES: return max_kw_of<EPI_RES, false>(mt, nt);
        case LGEN_EPI_SWIGLU: return fused_norm ? max_kw_of<EPI_SWIGLU, true>(mt, nt) : max_kw_of<EPI_SWIGLU, false>(mt, nt);
        case LGEN_EPI_QKV: return fused_norm ? max_kw_of<EPI_QKV, true>(mt, nt) : max_kw_of<EPI_QKV, false>(mt, nt);
        default: return 0;
    }
}

extern "C" int lgen_gemm(const void* wp, const void* xp, void* out, int M, int MTs, int N, int K, int epilogue_kind,
                         int dtype, int mt, int nt, int kw, const void* norm_w, const float* ssq_in, int ssq_parts,
                         float eps, float* ssq_out, int passes, void* stream) {
    const int kcsz = kc_of(dtype);
    if (N % 16 || K % kcsz || M > MTs * 16 || passes < 1 || passes > 64) return LGEN_ERR_BAD_ARG;
    if ((norm_w && (ssq_parts < 1 || ssq_parts > LGEN_SSQ_STRIDE)) || (ssq_out && N / 16 > LGEN_SSQ_STRIDE)) return LGEN_ERR_BAD_ARG;
    GemmArgs a{};
    a.wp = (const uint4*)wp; a.xp = (const uint4*)xp; a.out = out;
    a.N = N; a.KCH = K / kcsz; a.MTs = MTs; a.M = M;
    a.nw = (const uint4*)norm_w; a.ssq_in = ssq_in; a.parts = ssq_parts; a.eps = eps; a.inv_k = 1.0f / (float)K;
    a.ssq_out = ssq_out;
    a.passes = passes;
    hipStream_t st = (hipStream_t)stream;
    if (ssq_out && epilogue_kind != LGEN_EPI_RES) return LGEN_ERR_BAD_ARG;
    switch (epilogue_kind) {
        case LGEN_EPI_ROWS: return dispatch_norm<EPI_ROWS>(a, dtype, mt, nt, kw, st);
        case LGEN_EPI_PACKED: return dispatch_norm<EPI_PACKED>(a, dtype, mt, nt, kw, st);
        case LGEN_EPI_GELU: return dispatch_norm<EPI_GELU>(a, dtype, mt, nt, kw, st);
        case LGEN_EPI_RES: return dispatch_norm<EPI_RES>(a, dtype, mt, nt, kw, st);
        case LGEN_EPI_SWIGLU: return dispatch_norm<EPI_SWIGLU>(a, dtype, mt, nt, kw, st);
        default: return LGEN_ERR_BAD_ARG;
    }
}

static int qkv_rope_impl(const void* wp, const void* xp, void* q_out, void* k_cache, void* v_cache, const float* freqs,
                         const int* pos_ptr, int pos_stride, int M, int MTs, int d, int n_head, int hd, int hdp, int S8,
                         int kv_row_stride, int dtype, int mt, int nt, int kw, const void* norm_w, const float* ssq_in,
                         int ssq_parts, float eps, int passes, void* stream, bool kv8 = false, float k_inv = 1.f, float v_inv = 1.f) {
    const int kcsz = kc_of(dtype);
    if (kv8 && (dtype != LGEN_BF16 || hdp != 64)) return LGEN_ERR_UNSUPPORTED;
    if (d % kcsz || (3 * d) % 16 || hd % 4 || d != n_head * hd || M > MTs * 16 || pos_stride < 0 || pos_stride > 1 || passes < 1 ||
        passes > 64)
        return LGEN_ERR_BAD_ARG;
    if (norm_w && (ssq_parts < 1 || ssq_parts > LGEN_SSQ_STRIDE)) return LGEN_ERR_BAD_ARG;
    GemmArgs a{};
    a.wp = (const uint4*)wp; a.xp = (const uint4*)xp; a.out = q_out; a.kc = k_cache; a.vc = v_cache;
    a.freqs = freqs; a.pos_ptr = pos_ptr; a.pos_stride = pos_stride;
    a.N = 3 * d; a.KCH = d / kcsz; a.MTs = MTs; a.M = M;
    a.d = d; a.hd = hd; a.hdp = hdp; a.H = n_head; a.S8 = S8;
    a.kvs = kv_row_stride > 0 ? kv_row_stride : hdp;
    a.k_inv = k_inv; a.v_inv = v_inv;
    {   // rows may be packed tighter than the lane group hdp (lgen.h): at least hd rounded up to one 16-byte piece of the storage type
        // (fp8 slabs: the stride is in bytes and the piece the attention loads is 8 bytes = 8 elements)
        const int epl_ = epl_of(dtype);
        if (a.kvs < (hd + epl_ - 1) / epl_ * epl_ || a.kvs % epl_) return LGEN_ERR_BAD_ARG;
    }
    a.nw = (const uint4*)norm_w; a.ssq_in = ssq_in; a.parts = ssq_parts; a.eps = eps; a.inv_k = 1.0f / (float)d;
    a.passes = passes;
    if (kv8) return dispatch_norm<EPI_QKV8>(a, dtype, mt, nt, kw, (hipStream_t)stream);
    return dispatch_norm<EPI_QKV>(a, dtype, mt, nt, kw, (hipStream_t)stream);
}

extern "C" int lgen_gemm_qkv_rope(const void* wp, const void* xp, void* q_out, void* k_cache, void* v_cache,
                                  const float* freqs, const int* pos_ptr, int M, int MTs, int d, int n_head, int hd,
                                  int hdp, int S8, int kv_row_stride, int dtype, int mt, int nt, int kw,
                                  const void* norm_w, const float* ssq_in, int ssq_parts, float eps, int passes, void* stream) {
    return qkv_rope_impl(wp, xp, q_out, k_cache, v_cache, freqs, pos_ptr, 0, M, MTs, d, n_head, hd, hdp, S8, kv_row_stride, dtype,
                         mt, nt, kw, norm_w, ssq_in, ssq_parts, eps, passes, stream);
}

extern "C" int lgen_gemm_qkv_rope_rows(const void* wp, const void* xp, void* q_out, void* k_cache, void* v_cache,
                                       const float* freqs, const int* row_pos, int M, int MTs, int d, int n_head, int hd,
                                       int hdp, int S8, int kv_row_stride, int dtype, int mt, int nt, int kw,
                                       const void* norm_w, const float* ssq_in, int ssq_parts, float eps, int passes, void* stream) {
    return qkv_rope_impl(wp, xp, q_out, k_cache, v_cache, freqs, row_pos, 1, M, MTs, d, n_head, hd, hdp, S8, kv_row_stride, dtype,
                         mt, nt, kw, norm_w, ssq_in, ssq_parts, eps, passes, stream);
}

extern "C" int lgen_gemm_qkv_rope_kv8(const void* wp, const void* xp, void* q_out, void* k_cache, void* v_cache,
                                      const float* freqs, const int* pos_ptr, int M, int MTs, int d, int n_head, int hd,
                                      int hdp, int S8, int kv_row_stride, int dtype, int mt, int nt, int kw,
                                      const void* norm_w, const float* ssq_in, int ssq_parts, float eps, int passes,
                                      float k_inv_scale, float v_inv_scale, void* stream) {
    return qkv_rope_impl(wp, xp, q_out, k_cache, v_cache, freqs, pos_ptr, 0, M, MTs, d, n_head, hd, hdp, S8, kv_row_stride, dtype,
                         mt, nt, kw, norm_w, ssq_in, ssq_parts, eps, passes, stream, true, k_inv_scale, v_inv_scale);
}
