// composite_ray_body.inc - the body of composite_ray / composite_ray_mode (composite_dev.inc): render_core's tail for one ray on one wave.
// Included inside those two functions only; C, COH and MODE are theirs.
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
            av[i] = FADD(clipf(FADD(FSUB(1.0f, occ), FMUL(a.flip_sat, vis_mask)), 0.0f, 1.0f), 1e-7f);  // :515
        }
        ray_prefix_prod<C>(av, ok, sb);     // vis_prob (:511-523)
#pragma unroll
        for (int i = 0; i < C; ++i) {
            const float vp = clipf(sb[i], 0.0f, 1.0f);                                      // :528
            const float tcn = -fabsf(tc[i]);
            const float ap = sdf2alpha(u[i], tcn, dists[i], inv_s_, a.anneal != 0, a.car);  // :530-543
            const float am = sdf2alpha(-u[i], tcn, dists[i], inv_s_, a.anneal != 0, a.car);
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
