// Fused sequence scoring: log-probability of a GIVEN token under each row of storage-dtype logits.
//
//   out[r] = log_softmax(mix(row r) / max(temperature, 1e-5))[targets[r]]
//
// Replaces, for scoring, the fp32 [B, S, V] logits + F.cross_entropy of autoregressive/models/gpt.py:373-380 and the
// log_softmax + gather of autoregressive/serve/sampler.py:88-93,119-123 (no top-k / top-p here: a filtered target would be -inf).
// mix is the guidance mix of serve/sampler.py:54-58 (uncond + (cond - uncond) * cfg_scale, uncond = row r + pair_offset).
//
// One workgroup (256 threads) per row.  Thread t walks the 8-element pieces t, t + 256, ... of the row (16-byte loads; a wave reads
// a contiguous 1 KiB / 2 KiB run) and keeps an online (max, sum of exp) pair; the pairs merge over the wave by butterfly and over
// the 4 waves through 8 floats of LDS.  Nothing of width V is ever stored: the kernel reads R * V elements once and writes R floats.
#include "lgen_common.h"
#include "../../include/lgen.h"

#define LP_THREADS 256
#define LP_MAXV 16384

// (m, s) <- merge of two online-softmax partials; an empty partial is (-inf, 0) and merges without a NaN.  The two products are
// opaque values: left alone, the vectoriser pairs them into one packed-fp32 multiply and adds the halves with a packed add that
// reads the high register into the low result -- the crossed form tools/isa_lint.py bans (lgen_common.h: rope_pair).
LGEN_DEV void lp_merge(float& m, float& s, float om, float os) {
    const float M = fmaxf(m, om);
    float a = s * (m == M ? 1.f : expf(m - M)), b = os * (om == M ? 1.f : expf(om - M));
    asm volatile("" : "+v"(a), "+v"(b));
    s = a + b;
    m = M;
}

template <typename D>
__global__ __launch_bounds__(LP_THREADS) void logprob_rows_kernel(const void* __restrict__ logits, const int* __restrict__ targets,
                                                                  float* __restrict__ out, int V, int pair_offset, float cfg_scale,
                                                                  float tdiv, int mix) {
    __shared__ float red_m[LP_THREADS / 64], red_s[LP_THREADS / 64];
    __shared__ float sh_t;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r = blockIdx.x;
    const int tgt = targets[r];
    if (tgt < 0) {  // uniform over the workgroup: the row is not read
        if (tid == 0) out[r] = 0.f;
        return;
    }
    float m = -INFINITY, s = 0.f;
    for (int i0 = tid * 8; i0 < V; i0 += LP_THREADS * 8) {  // V % 8 == 0: a piece is inside the row or not at all
        float v[8], u[8];
        D::ld8(logits, (size_t)r * V + i0, v);
        if (mix) D::ld8(logits, (size_t)(r + pair_offset) * V + i0, u);
        float cm = -INFINITY;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float x = v[e];
            if (mix) x = u[e] + (x - u[e]) * cfg_scale;
            x = x / tdiv;
            v[e] = x;
            cm = fmaxf(cm, x);
        }
        if ((unsigned)(tgt - i0) < 8u) {  // this piece holds the target: exactly one thread, once
            float t = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (e == tgt - i0) t = v[e];
            sh_t = t;
        }
        if (cm > m) { s *= expf(m - cm); m = cm; }  // first piece: s == 0 and expf(-inf) == 0
        float acc = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {  // (opaque running sum: no packed horizontal add here either)
            acc += expf(v[e] - m);
            asm volatile("" : "+v"(acc));
        }
        s += acc;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lp_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
    if (lane == 0) { red_m[wv] = m; red_s[wv] = s; }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < LP_THREADS / 64; ++i) lp_merge(m, s, red_m[i], red_s[i]);
        out[r] = (sh_t - m) - logf(s);
    }
}

extern "C" int lgen_logprob_rows(const void* logits, const int* targets, float* out, int R, int V, int pair_offset,
                                 float cfg_scale, float temperature, int dtype, void* stream) {
    if (!logits || !targets || !out || R < 1 || V < 8 || (V & 7) || V > LP_MAXV || pair_offset < 0) return LGEN_ERR_BAD_ARG;
    const int mix = pair_offset > 0 && cfg_scale > 1.0f;
    const float tdiv = fmaxf(temperature, 1e-5f);
    return lgen_dispatch_dtype(dtype, [&](auto tag) {
        hipLaunchKernelGGL(logprob_rows_kernel<decltype(tag)>, dim3(R), dim3(LP_THREADS), 0, (hipStream_t)stream, logits, targets,
                           out, V, pair_offset, cfg_scale, tdiv, mix);
        LGEN_CHECK_LAUNCH();
        return 0;
    });
}
