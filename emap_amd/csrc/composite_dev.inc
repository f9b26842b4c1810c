// composite_dev.inc - render_core's tail (udf_renderer_blending.py:435-455,463-677) for ONE ray on one 64-lane wave, shared by
// composite_kernel (sampler.hip: one workgroup per ray) and by the value + grad_x kernel's fused tail (udf_mlp_rev32.inc, COMP: the
// workgroup that completes a ray's last tile composites it - BASELINE config C2's "fused MLP + composite").  Included inside namespace emap,
// after sampler_dev.inc.
#pragma once

// COH: udf / grad_x were written by OTHER workgroups of the running kernel (possibly behind another XCD's L2) with agent-scope stores
// (global_store ... sc1); read them with agent-scope loads (global_load ... sc1), never through this XCD's possibly stale L2 lines.
template <bool COH>
__device__ __forceinline__ float comp_ld(const float* p) {
    if constexpr (COH) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}

// Round 5: the ray lives in registers (lane l = samples [l C, (l+1) C), C = 1, 2 or 4), one burst of loads, neighbours over DPP, no LDS and
// no barriers - see composite_bwd_kernel.  Same expressions and the same scan chunks as the LDS version of rounds 1-4.
// MODE (compile time, EmapRenderParams.render_mode): EMAP_RENDER_UNBIASED (use_unbias_render=True, :479-549), EMAP_RENDER_UNBIASED_NORMCOS
// (the same with use_norm_grad_for_cosine=True: true_cos from the normalised gradient, :479-480) or EMAP_RENDER_PLAIN (use_unbias_render=False,
// :551-559: alpha = alpha_occ, gradients_flip = gradients, :635-639).  The body (composite_ray_body.inc) is included twice: composite_ray is
// the default mode under its own name and template signature, so that the code of the fused tail of udf_mlp_rev32.inc (COH = true, the
// default mode only) stays what it was to the byte; composite_ray_mode is the separate compositing launch of every mode.
template <int C, bool COH>
__device__ __forceinline__ void composite_ray(const CompositeArgs& a, const int ray, const int lane) {
    constexpr int MODE = EMAP_RENDER_UNBIASED;
#include "composite_ray_body.inc"
}

template <int C, int MODE>
__device__ __forceinline__ void composite_ray_mode(const CompositeArgs& a, const int ray, const int lane) {
    constexpr bool COH = false;
#include "composite_ray_body.inc"
}

// deterministic cross-ray reduction of the eikonal terms (:618-625) and sparse_error (:642-644)
// COH: the partials were written by other workgroups of the RUNNING launch (agent-scope stores above): agent-scope loads.  Same additions in the same order
// either way (thread t takes rays t, t + nthreads, ...; lanes, then waves in order): the launch that composited the rays can finish the render itself.
template <bool COH>
__device__ __forceinline__ void composite_reduce_body(const float* partials, int N, float* scalars, int32_t* err, const CompositeArgs& a, int tid, int nthreads,
                                                      double (*red)[5]) {
    const int nw = nthreads >> 6;
    double v[5] = {0, 0, 0, 0, 0};
    typedef float f4 __attribute__((ext_vector_type(4)));
    for (int i = tid; i < N; i += nthreads) {
        f4 lo;
        float hi;
        if constexpr (COH) {
            const float* q = partials + (size_t)i * 8;
            lo = f4{comp_ld<true>(q), comp_ld<true>(q + 1), comp_ld<true>(q + 2), comp_ld<true>(q + 3)};
            hi = comp_ld<true>(q + 4);
        } else {
            lo = *reinterpret_cast<const f4*>(partials + (size_t)i * 8);
            hi = partials[(size_t)i * 8 + 4];
        }
        v[0] += (double)lo[0]; v[1] += (double)lo[1]; v[2] += (double)lo[2]; v[3] += (double)lo[3]; v[4] += (double)hi;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = wave_sum_d(v[k]);
    if ((tid & 63) == 0)
#pragma unroll
        for (int k = 0; k < 5; ++k) red[tid >> 6][k] = v[k];
    __syncthreads();
    if (tid == 0) {
        double t[5];
        for (int k = 0; k < 5; ++k) { t[k] = 0; for (int q = 0; q < nw; ++q) t[k] += red[q][k]; }
        const float e_rel = (float)t[0], c_rel = (float)t[1], e_ns = (float)t[2], c_ns = (float)t[3];
        const float ge = FDIV(e_rel, FADD(c_rel, 1e-5f));
        scalars[0] = ge;
        scalars[1] = FDIV(e_ns, FADD(c_ns, 1e-5f));
        scalars[2] = (float)(t[4] / (double)N);
        scalars[3] = e_rel; scalars[4] = c_rel; scalars[5] = e_ns; scalars[6] = c_ns; scalars[7] = (float)t[4];
        // s_val = 1/inv_s, 1/beta, gamma: the "variance"/"beta"/"gamma" entries of the render dict (:656-658)
        float inv_s_ = a.inv_s, beta_ = a.beta, gamma_ = a.gamma;
        if (a.var_p) {
            inv_s_ = clipf(expf(FMUL(a.var_p[0], 10.0f)), 1e-6f, 1e6f);
            beta_ = clipf(clipf(expf(FMUL(a.beta_p[0], 10.0f)), 0.0f, FDIV(1.0f, a.beta_min)), 1e-6f, 1e6f);
            gamma_ = clipf(expf(FMUL(a.gamma_p[0], 10.0f)), 1e-6f, 1e6f);
        }
        scalars[8] = FDIV(1.0f, inv_s_); scalars[9] = FDIV(1.0f, beta_); scalars[10] = gamma_; scalars[11] = inv_s_;
        if (err && ge != ge) atomicOr(err, EMAP_F_NAN_GRADERR);
    }
}

