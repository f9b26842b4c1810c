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
// :551-559: alpha = alpha_occ, gradients_flip = gradients, :635-639).  composite_kernel (sampler.hip) runs every mode with COH = false; the fused
// tail of udf_mlp_rev32.inc runs the default mode with COH = true.
template <int C, bool COH, int MODE = EMAP_RENDER_UNBIASED>
__device__ __forceinline__ void composite_ray(const CompositeArgs& a, const int ray, const int lane) {
    const int S = a.S;
    const size_t rb = (size_t)ray * S;
    float z[C + 1], u[C], gx[C], gy[C], gz[C], tc[C + 1];
    bool ok[C], last[C];
#pragma unroll
    for (int i = 0; i < C; ++i) {
        const int e = lane * C + i;
        ok[i] = e < S; last[i] = !(e < S - 1);
        const size_t q = rb + (ok[i] ? e : S - 1);
        z[i] = a.z[q]; u[i] = comp_ld<COH>(a.udf + q);
        gx[i] = comp_ld<COH>(a.grad + 3 * q); gy[i] = comp_ld<COH>(a.grad + 3 * q + 1); gz[i] = comp_ld<COH>(a.grad + 3 * q + 2);
    }
    const float ox = a.rays_o[3 * ray], oy = a.rays_o[3 * ray + 1], oz = a.rays_o[3 * ray + 2];
    const float dx = a.rays_d[3 * ray], dy = a.rays_d[3 * ray + 1], dz = a.rays_d[3 * ray + 2];
    const float sd = *a.sample_dist;
    // cos_anneal_ratio / flip_saturation of this step: from the schedule kernel's device words where the caller fed them (uniform loads)
    const float car = a.sched ? a.sched[2] : a.car, flip_sat = a.sched ? a.sched[3] : a.flip_sat;
    float inv_s_ = a.inv_s, beta_ = a.beta, gamma_ = a.gamma;
    if (a.var_p) {  // udf_model.py:226-227,259-263 + udf_renderer_blending.py:466-472
        inv_s_ = clipf(expf(FMUL(a.var_p[0], 10.0f)), 1e-6f, 1e6f);
        beta_ = clipf(clipf(expf(FMUL(a.beta_p[0], 10.0f)), 0.0f, FDIV(1.0f, a.beta_min)), 1e-6f, 1e6f);
        gamma_ = clipf(expf(FMUL(a.gamma_p[0], 10.0f)), 1e-6f, 1e6f);
    }
    if constexpr (MODE == EMAP_RENDER_UNBIASED_NORMCOS) {
#pragma unroll
        for (int i = 0; i < C; ++i) {       // :463-464,480: dirs . (g / (|g| + 1e-5)), the expression of cosn below
            const float gi = FADD(sqrtf(FADD(FADD(FMUL(gx[i], gx[i]), FMUL(gy[i], gy[i])), FMUL(gz[i], gz[i]))), 1e-5f);
            tc[i] = FADD(FADD(FMUL(dx, FDIV(gx[i], gi)), FMUL(dy, FDIV(gy[i], gi))), FMUL(dz, FDIV(gz[i], gi)));
        }
    } else if constexpr (MODE == EMAP_RENDER_UNBIASED) {
#pragma unroll
        for (int i = 0; i < C; ++i) tc[i] = FADD(FADD(FMUL(dx, gx[i]), FMUL(dy, gy[i])), FMUL(dz, gz[i]));      // :482
    }
    z[C] = dpp_next_f(0.f, z[0]);       // sample e+1 of a lane's last sample is the next lane's first
    if constexpr (MODE != EMAP_RENDER_PLAIN) tc[C] = dpp_next_f(0.f, tc[0]);
    float dists[C], av[C], sb[C];
    float alpha[C];
    if constexpr (MODE == EMAP_RENDER_PLAIN) {
#pragma unroll
        for (int i = 0; i < C; ++i) {
            dists[i] = last[i] ? sd : FSUB(z[i + 1], z[i]);                             // :435-444
            const float raw_occ = udf2logistic1(u[i], beta_);                           // :553-558
            alpha[i] = FSUB(1.0f, expf(FMUL(FMUL(-relu_(raw_occ), gamma_), dists[i])));    // :559
            av[i] = FADD(FSUB(1.0f, alpha[i]), 1e-7f);
        }
    } else {
#pragma unroll
        for (int i = 0; i < C; ++i) {
            dists[i] = last[i] ? sd : FSUB(z[i + 1], z[i]);                                 // :435-444
            const float raw_occ = udf2logistic1(u[i], beta_);                               // :492
            const float occ = FSUB(1.0f, expf(FMUL(FMUL(-relu_(raw_occ), gamma_), dists[i])));   // :497
            const float vis_mask = last[i] ? 1.0f : ((tc[i + 1] < 0.01f) ? 1.0f : 0.0f);    // :500-509
            av[i] = FADD(clipf(FADD(FSUB(1.0f, occ), FMUL(flip_sat, vis_mask)), 0.0f, 1.0f), 1e-7f);  // :515
        }
        ray_prefix_prod<C>(av, ok, sb);     // vis_prob (:511-523)
#pragma unroll
        for (int i = 0; i < C; ++i) {
            const float vp = clipf(sb[i], 0.0f, 1.0f);                                      // :528
            const float tcn = -fabsf(tc[i]);
            const float ap = sdf2alpha(u[i], tcn, dists[i], inv_s_, a.anneal != 0, car);  // :530-543
            const float am = sdf2alpha(-u[i], tcn, dists[i], inv_s_, a.anneal != 0, car);
            alpha[i] = FADD(FMUL(ap, vp), FMUL(am, FSUB(1.0f, vp)));                        // :545
            av[i] = FADD(FSUB(1.0f, alpha[i]), 1e-7f);
        }
    }
    ray_prefix_prod<C>(av, ok, sb);     // transmittance (:593-602)
    double wsum = 0, dsum = 0, nx = 0, ny = 0, nz = 0, e_rel = 0, c_rel = 0, e_ns = 0, c_ns = 0, sp = 0;
#pragma unroll
    for (int i = 0; i < C; ++i) {
        const float w = FMUL(alpha[i], sb[i]);
        const float mid = FADD(z[i], FMUL(dists[i], 0.5f));                             // :446
        const float px = FADD(ox, FMUL(dx, mid)), py = FADD(oy, FMUL(dy, mid)), pz = FADD(oz, FMUL(dz, mid));
        const float pn = sqrtf(FADD(FADD(FMUL(px, px), FMUL(py, py)), FMUL(pz, pz)));   // :563
        const float gm = sqrtf(FADD(FADD(FMUL(gx[i], gx[i]), FMUL(gy[i], gy[i])), FMUL(gz[i], gz[i])));   // :463
        const float gi = FADD(gm, 1e-5f);
        const float cosn = FADD(FADD(FMUL(dx, FDIV(gx[i], gi)), FMUL(dy, FDIV(gy[i], gi))), FMUL(dz, FDIV(gz[i], gi)));  // :485
        const float flip = (MODE == EMAP_RENDER_PLAIN) ? 1.0f : ((cosn > 0.f) ? -1.0f : 1.0f);   // :486-489; plain: :639
        const float inside = (pn < 2.0f) ? 1.0f : 0.0f, relax = (pn < 2.4f) ? 1.0f : 0.0f;  // :568-569
        const float ns = (u[i] < a.near_surface) ? 1.0f : 0.0f;                         // :570
        const float ge = FMUL(FSUB(gm, 1.0f), FSUB(gm, 1.0f));                          // :612-617
        if (ok[i]) {
            const size_t q = rb + lane * C + i;
            if (a.out.weights) a.out.weights[q] = w;
            if (a.out.alpha) a.out.alpha[q] = alpha[i];
            if (a.out.mid_z) a.out.mid_z[q] = mid;
            if (a.out.dists) a.out.dists[q] = dists[i];
            if (a.out.inside_sphere) a.out.inside_sphere[q] = inside;
            if (a.out.gradient_mag) a.out.gradient_mag[q] = gm;
            if (a.out.gradients_flip) {
                a.out.gradients_flip[3 * q] = FMUL(flip, gx[i]);
                a.out.gradients_flip[3 * q + 1] = FMUL(flip, gy[i]);
                a.out.gradients_flip[3 * q + 2] = FMUL(flip, gz[i]);
            }
            wsum += w;
            dsum += (double)FMUL(mid, w);
            nx += (double)FMUL(FMUL(flip, gx[i]), w); ny += (double)FMUL(FMUL(flip, gy[i]), w); nz += (double)FMUL(FMUL(flip, gz[i]), w);
            e_rel += (double)FMUL(relax, ge); c_rel += relax;
            e_ns += (double)FMUL(ns, ge); c_ns += ns;
            sp += (double)expf(FMUL(-a.sparse_scale, u[i]));                            // :642-644
        }
    }
    wsum = wave_sum_d(wsum); dsum = wave_sum_d(dsum);
    nx = wave_sum_d(nx); ny = wave_sum_d(ny); nz = wave_sum_d(nz);
    e_rel = wave_sum_d(e_rel); c_rel = wave_sum_d(c_rel); e_ns = wave_sum_d(e_ns); c_ns = wave_sum_d(c_ns);
    sp = wave_sum_d(sp);
    if (lane == 0) {
        const float ws = (float)wsum;
        float edge = ws;                                                                 // :606 (sampled_edge == 1)
        if (a.has_bg) edge = FADD(edge, FMUL(a.background, FSUB(1.0f, ws)));             // :608-609
        if (a.out.edge) a.out.edge[ray] = edge;
        if (a.out.weight_sum) a.out.weight_sum[ray] = ws;
        if (a.out.depth) a.out.depth[ray] = a.depth_scale ? FMUL((float)dsum, a.depth_scale[ray]) : (float)dsum;  // :607, render :786
        if (a.out.normals) { a.out.normals[3 * ray] = (float)nx; a.out.normals[3 * ray + 1] = (float)ny; a.out.normals[3 * ray + 2] = (float)nz; }
        float* p = a.partials + (size_t)ray * 8;
        if constexpr (COH) {     // the cross-ray reduction may run in ANOTHER workgroup of this launch (composite_reduce_body<true>): write through to the coherence point
            __hip_atomic_store(p + 0, (float)e_rel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(p + 1, (float)c_rel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(p + 2, (float)e_ns, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(p + 3, (float)c_ns, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(p + 4, (float)sp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            p[0] = (float)e_rel; p[1] = (float)c_rel; p[2] = (float)e_ns; p[3] = (float)c_ns; p[4] = (float)sp;
        }
    }
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

