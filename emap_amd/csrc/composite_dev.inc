// composite_dev.inc - render_core's tail (udf_renderer_blending.py:435-455,463-677) for ONE ray on one 64-lane wave.  composite_forward is the
// tail up to the transmittance, written once: composite_ray (forward + outputs: composite_kernel in sampler.hip, one workgroup per ray, and the
// value + grad_x kernel's fused tail in udf_mlp_rev32.inc, COMP: the workgroup that completes a ray's last tile composites it - BASELINE config
// C2's "fused MLP + composite") and composite_bwd_kernel (forward + adjoint, sampler.hip) both run it.  Included inside namespace emap, after
// sampler_dev.inc.
#pragma once

// COH: udf / grad_x were written by OTHER workgroups of the running kernel (possibly behind another XCD's L2) with agent-scope stores
// (global_store ... sc1); read them with agent-scope loads (global_load ... sc1), never through this XCD's possibly stale L2 lines.
template <bool COH>
__device__ __forceinline__ float comp_ld(const float* p) {
    if constexpr (COH) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}

// inv_s / beta / gamma (udf_model.py:226-227,259-263 + udf_renderer_blending.py:466-472) and cos_anneal_ratio / flip_saturation of this
// launch: by value, or from the raw device parameters x = exp(10 p) (then x_* holds them before the clips: the adjoint's reduction passes a
// gradient on only where clipped == x) and from the schedule kernel's device words where the caller fed them (uniform loads).
struct RenderScalars { float inv_s, beta, gamma, car, flip_sat, x_var, x_beta, x_gamma; };
__device__ __forceinline__ RenderScalars render_scalars(const CompositeCore& a) {
    RenderScalars s{a.inv_s, a.beta, a.gamma, a.sched ? a.sched[2] : a.car, a.sched ? a.sched[3] : a.flip_sat, 0.f, 0.f, 0.f};
    if (a.var_p) {
        s.x_var = expf(FMUL(a.var_p[0], 10.0f)); s.x_beta = expf(FMUL(a.beta_p[0], 10.0f)); s.x_gamma = expf(FMUL(a.gamma_p[0], 10.0f));
        s.inv_s = clipf(s.x_var, 1e-6f, 1e6f);
        s.beta = clipf(clipf(s.x_beta, 0.0f, FDIV(1.0f, a.beta_min)), 1e-6f, 1e6f);
        s.gamma = clipf(s.x_gamma, 1e-6f, 1e6f);
    }
    return s;
}

// One ray of render_core's tail up to the transmittance, in registers: lane l holds the C = 1, 2, 4 (8, 16: S > 256) consecutive samples
// [l C, (l+1) C) (the chunking wave_scan uses), every input is fetched by one burst of loads at the top, neighbours (z, true_cos of sample
// e+1) come over the DPP network, the two prefix products are fp64 wave scans.  No LDS, no barriers.  ok / last: the sample exists / is the
// ray's last one (lanes past the end hold copies of it).
// ADJ: what only the adjoint (sampler.hip:composite_bwd_kernel) reads - ain (the visibility factor before its clip), vp, ap, am and, for
// C <= 4 (KEEP), the pieces of occ_opacity, sdf2alpha_keep and norm_cos per sample; for C >= 8 they do not all stay in registers and the
// adjoint evaluates them again.  Without ADJ nothing is stored there.
template <int C, bool ADJ>
struct RayForward {
    static constexpr bool KEEP = ADJ && C <= 4;
    static constexpr int CA = ADJ ? C : 1, CK = KEEP ? C : 1;
    float z[C + 1], u[C], gx[C], gy[C], gz[C], tc[C + 1];
    bool ok[C], last[C];
    float ox, oy, oz, dx, dy, dz;
    RenderScalars s;
    float dists[C], av[C], vpr[C], alpha[C], om[C], T[C];   // vpr: the raw (unclipped) visibility product of av; T: transmittance, of om
    float ain[CA], vp[CA], ap[CA], am[CA];
    OccOpacity oc[CK];
    Sdf2AlphaKeep kp[CK], km[CK];
    float gi[CK];
};

// MODE (compile time, EmapRenderParams.render_mode): EMAP_RENDER_UNBIASED (use_unbias_render=True, :479-549), EMAP_RENDER_UNBIASED_NORMCOS
// (the same with use_norm_grad_for_cosine=True: true_cos from the normalised gradient, :479-480) or EMAP_RENDER_PLAIN (use_unbias_render=False,
// :551-559: alpha = alpha_occ, gradients_flip = gradients, :635-639).  composite_kernel and composite_bwd_kernel (sampler.hip) run every mode
// with COH = false; the fused tail of udf_mlp_rev32.inc runs the default mode with COH = true.
template <int C, bool COH, int MODE, bool ADJ>
__device__ __forceinline__ RayForward<C, ADJ> composite_forward(const CompositeCore& a, const int ray, const int lane) {
    constexpr bool KEEP = RayForward<C, ADJ>::KEEP;
    RayForward<C, ADJ> f;
    const int S = a.S;
    const size_t rb = (size_t)ray * S;
#pragma unroll
    for (int i = 0; i < C; ++i) {
        const int e = lane * C + i;
        f.ok[i] = e < S; f.last[i] = !(e < S - 1);
        const size_t q = rb + (f.ok[i] ? e : S - 1);
        f.z[i] = a.z[q]; f.u[i] = comp_ld<COH>(a.udf + q);
        f.gx[i] = comp_ld<COH>(a.grad + 3 * q); f.gy[i] = comp_ld<COH>(a.grad + 3 * q + 1); f.gz[i] = comp_ld<COH>(a.grad + 3 * q + 2);
    }
    f.ox = a.rays_o[3 * ray]; f.oy = a.rays_o[3 * ray + 1]; f.oz = a.rays_o[3 * ray + 2];
    f.dx = a.rays_d[3 * ray]; f.dy = a.rays_d[3 * ray + 1]; f.dz = a.rays_d[3 * ray + 2];
    const float sd = *a.sample_dist;
    f.s = render_scalars(a);
    if constexpr (MODE == EMAP_RENDER_UNBIASED_NORMCOS) {
#pragma unroll
        for (int i = 0; i < C; ++i) {       // :463-464,480
            const NormCos n = norm_cos(f.dx, f.dy, f.dz, f.gx[i], f.gy[i], f.gz[i]);
            f.tc[i] = n.cos;
            if constexpr (KEEP) f.gi[i] = n.gi;
        }
    } else if constexpr (MODE == EMAP_RENDER_UNBIASED) {
#pragma unroll
        for (int i = 0; i < C; ++i) f.tc[i] = FADD(FADD(FMUL(f.dx, f.gx[i]), FMUL(f.dy, f.gy[i])), FMUL(f.dz, f.gz[i]));      // :482
    }
    f.z[C] = dpp_next_f(0.f, f.z[0]);       // sample e+1 of a lane's last sample is the next lane's first
    if constexpr (MODE != EMAP_RENDER_PLAIN) f.tc[C] = dpp_next_f(0.f, f.tc[0]);
#pragma unroll
    for (int i = 0; i < C; ++i) {
        f.dists[i] = f.last[i] ? sd : FSUB(f.z[i + 1], f.z[i]);                         // :435-444
        const OccOpacity o = occ_opacity(f.u[i], f.s.beta, f.s.gamma, f.dists[i]);      // :492-497; plain :553-558
        if constexpr (KEEP) f.oc[i] = o;
        if constexpr (MODE == EMAP_RENDER_PLAIN) {
            f.alpha[i] = FSUB(1.0f, o.eq);                                              // :559
        } else {
            const float occ = FSUB(1.0f, o.eq);
            const float vis_mask = f.last[i] ? 1.0f : ((f.tc[i + 1] < 0.01f) ? 1.0f : 0.0f);    // :500-509
            const float ain = FADD(FSUB(1.0f, occ), FMUL(f.s.flip_sat, vis_mask));
            if constexpr (ADJ) f.ain[i] = ain;
            f.av[i] = FADD(clipf(ain, 0.0f, 1.0f), 1e-7f);                              // :515
        }
    }
    if constexpr (MODE != EMAP_RENDER_PLAIN) ray_prefix_prod<C>(f.av, f.ok, f.vpr);     // vis_prob (:511-523)
#pragma unroll
    for (int i = 0; i < C; ++i) {
        if constexpr (MODE != EMAP_RENDER_PLAIN) {
            const float vp = clipf(f.vpr[i], 0.0f, 1.0f);                               // :528
            const float tcn = -fabsf(f.tc[i]);
            Sdf2AlphaKeep kp, km;
            const float ap = sdf2alpha_keep(f.u[i], tcn, f.dists[i], f.s.inv_s, a.anneal != 0, f.s.car, kp);   // :530-543
            const float am = sdf2alpha_keep(-f.u[i], tcn, f.dists[i], f.s.inv_s, a.anneal != 0, f.s.car, km);
            f.alpha[i] = FADD(FMUL(ap, vp), FMUL(am, FSUB(1.0f, vp)));                  // :545
            if constexpr (ADJ) { f.vp[i] = vp; f.ap[i] = ap; f.am[i] = am; }
            if constexpr (KEEP) { f.kp[i] = kp; f.km[i] = km; }
        }
        f.om[i] = FADD(FSUB(1.0f, f.alpha[i]), 1e-7f);
    }
    ray_prefix_prod<C>(f.om, f.ok, f.T);    // transmittance (:593-602)
    return f;
}

// composite_forward + render_core's outputs and per-ray reductions: the body of composite_kernel (sampler.hip: one workgroup per ray) and of
// the fused tail of udf_mlp_rev32.inc
template <int C, bool COH, int MODE = EMAP_RENDER_UNBIASED>
__device__ __forceinline__ void composite_ray(const CompositeArgs& a, const int ray, const int lane) {
    const RayForward<C, false> f = composite_forward<C, COH, MODE, false>(a, ray, lane);
    const size_t rb = (size_t)ray * a.S;
    double wsum = 0, dsum = 0, nx = 0, ny = 0, nz = 0, e_rel = 0, c_rel = 0, e_ns = 0, c_ns = 0, sp = 0;
#pragma unroll
    for (int i = 0; i < C; ++i) {
        const float w = FMUL(f.alpha[i], f.T[i]);
        const float mid = FADD(f.z[i], FMUL(f.dists[i], 0.5f));                         // :446
        const float px = FADD(f.ox, FMUL(f.dx, mid)), py = FADD(f.oy, FMUL(f.dy, mid)), pz = FADD(f.oz, FMUL(f.dz, mid));
        const float pn = sqrtf(FADD(FADD(FMUL(px, px), FMUL(py, py)), FMUL(pz, pz)));   // :563
        const NormCos n = norm_cos(f.dx, f.dy, f.dz, f.gx[i], f.gy[i], f.gz[i]);        // :463, :485
        const float gm = n.gm;
        const float flip = (MODE == EMAP_RENDER_PLAIN) ? 1.0f : ((n.cos > 0.f) ? -1.0f : 1.0f);   // :486-489; plain: :639
        const float inside = (pn < 2.0f) ? 1.0f : 0.0f, relax = (pn < 2.4f) ? 1.0f : 0.0f;  // :568-569
        const float ns = (f.u[i] < a.near_surface) ? 1.0f : 0.0f;                       // :570
        const float ge = FMUL(FSUB(gm, 1.0f), FSUB(gm, 1.0f));                          // :612-617
        if (f.ok[i]) {
            const size_t q = rb + lane * C + i;
            if (a.out.weights) a.out.weights[q] = w;
            if (a.out.alpha) a.out.alpha[q] = f.alpha[i];
            if (a.out.mid_z) a.out.mid_z[q] = mid;
            if (a.out.dists) a.out.dists[q] = f.dists[i];
            if (a.out.inside_sphere) a.out.inside_sphere[q] = inside;
            if (a.out.gradient_mag) a.out.gradient_mag[q] = gm;
            if (a.out.gradients_flip) {
                a.out.gradients_flip[3 * q] = FMUL(flip, f.gx[i]);
                a.out.gradients_flip[3 * q + 1] = FMUL(flip, f.gy[i]);
                a.out.gradients_flip[3 * q + 2] = FMUL(flip, f.gz[i]);
            }
            wsum += w;
            dsum += (double)FMUL(mid, w);
            nx += (double)FMUL(FMUL(flip, f.gx[i]), w); ny += (double)FMUL(FMUL(flip, f.gy[i]), w); nz += (double)FMUL(FMUL(flip, f.gz[i]), w);
            e_rel += (double)FMUL(relax, ge); c_rel += relax;
            e_ns += (double)FMUL(ns, ge); c_ns += ns;
            sp += (double)expf(FMUL(-a.sparse_scale, f.u[i]));                          // :642-644
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
        const RenderScalars s = render_scalars(a);
        scalars[8] = FDIV(1.0f, s.inv_s); scalars[9] = FDIV(1.0f, s.beta); scalars[10] = s.gamma; scalars[11] = s.inv_s;
        if (err && ge != ge) atomicOr(err, EMAP_F_NAN_GRADERR);
    }
}

