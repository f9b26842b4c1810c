// rays.hip - on-device ray / pixel sampler (SURVEY.md par. 8 f3).
//
// Replaces Dataset.gen_random_rays_patches_at (reference src/dataset/dataset.py:222-307): per training step the reference
// draws pixels on the HOST (torch.randint, and python `random.choices` over all H*W pixel probabilities when
// importance_sample=True), builds the rays with a handful of small torch CPU ops and copies six tensors to the GPU.  Once a
// render step takes well under a millisecond that host work dominates.  Here one kernel does all of it from data that
// lives on the device: pixel draw (Philox4x32-10 counter-based stream), edge look-up, p = K^-1 [x, y, 1], rays_v = R p/|p|,
// rays_o = t, depth_scale, ndc coordinates.  Zero host->device copies per step; the step counter itself is a device word, so
// the sampler can sit inside a captured hipGraph.
//
// Importance sampling (dataset.py:236-263): half of the batch uniform, half from `random.choices(pixels, probabilities)` with
// probabilities = 1 - d on pixels whose edge value is > 0.1 and d elsewhere (d = mean edge value of the image).  Two weight
// classes -> pick the class with probability mass n_e (1-d) : n_n d, then a uniform member of the class: exactly that
// distribution, from a per-image list of pixel indices with the edge pixels first (built once on upload).
// The host generators (torch CPU Mersenne / python random) cannot be reproduced on a device; parity is therefore (i) the
// deterministic part - rays of GIVEN pixels equal the reference formulas - and (ii) distribution tests (SURVEY par. 8c).
#include "emap_common.h"

namespace emap {

struct Philox {
    uint32_t k0, k1;
    __device__ __forceinline__ static void round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    }
    __device__ __forceinline__ static void gen(uint64_t seed, uint64_t stream, uint64_t index, uint32_t (&out)[4]) {
        uint32_t c[4] = {(uint32_t)index, (uint32_t)(index >> 32), (uint32_t)stream, (uint32_t)(stream >> 32)};
        uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            round(c, k0, k1);
            k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
        }
        out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
    }
};

// uniform integer in [0, n) from 32 random bits (multiply-shift; bias < n / 2^32)
__device__ __forceinline__ int rand_below(uint32_t r, int n) { return (int)(((uint64_t)r * (uint64_t)n) >> 32); }

// The training list of emap_sample_rays_train: position step % n of perm, which holds epoch step / n's order of `images` (null: perm is
// fixed).  `tag` is the epoch perm was computed for.
struct EpochArgs {
    const int32_t* images;
    int32_t* perm;
    int64_t* tag;
    int32_t n;               // 0: the launch is emap_sample_rays' (ds.image_perm, step % n_images)
};

struct RayArgs {
    EmapRayDataset ds;
    EmapRayBatch out;
    EpochArgs ep;
    const int64_t* pixels_in;
    const uint64_t* counter;
    uint64_t* bump;          // the counter again when THIS launch increments it (single-workgroup launches), else null
    uint64_t seed, offset;
    int32_t img_idx, batch, importance;
};

__device__ __forceinline__ void sample_ray(const RayArgs& a, uint64_t step, int i);

// The image order of epoch e = step / n, by ONE workgroup (every thread of it calls this): perm[j] = images[sigma(j)], sigma the stable
// argsort of the n keys Philox(seed, stream 2^63 | e, index i) words 0 (high) and 1 (low) - a stream the ray draws (stream = step < 2^63)
// never reach.  One lane per image (strided where the workgroup is smaller), rank = number of smaller keys.  Nothing happens while the
// buffer's tag is e already, so a step inside an epoch pays one load; a counter written from outside (resume, a capture's rollback)
// makes the tag differ and the order follows.
__device__ __forceinline__ void reshuffle_epoch(const EpochArgs& t, uint64_t seed, uint64_t step) {
    __shared__ uint64_t keys[EMAP_MAX_TRAIN_IMAGES];
    const uint64_t e = step / (uint64_t)t.n;
    if (*t.tag == (int64_t)e) return;                           // uniform; the tag is written behind two barriers below
    for (int i = threadIdx.x; i < t.n; i += blockDim.x) {
        uint32_t r[4];
        Philox::gen(seed, 0x8000000000000000ull | e, (uint64_t)i, r);
        keys[i] = ((uint64_t)r[0] << 32) | r[1];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < t.n; i += blockDim.x) {
        const uint64_t k = keys[i];
        int rank = 0;
        for (int j = 0; j < t.n; ++j) {
            const uint64_t kj = keys[j];
            rank += (kj < k || (kj == k && j < i)) ? 1 : 0;
        }
        t.perm[rank] = t.images[i];
    }
    __syncthreads();                                            // perm is complete (and visible to the workgroup) from here on
    if (threadIdx.x == 0) *t.tag = (int64_t)e;
}

// batch > 1024 only: the order is brought up to date by a launch of its own, ahead of the many-workgroup sample kernel
__global__ __launch_bounds__(1024) void reshuffle_epoch_kernel(const EpochArgs t, const uint64_t* counter, uint64_t seed) {
    reshuffle_epoch(t, seed, *counter);
}

// batch <= 1024: ONE workgroup, which also increments the step counter once every lane has read it (a second launch for that cost 4.8 us of
// a 6 us job); larger batches: 256-thread workgroups and bump_counter_kernel behind them
__global__ __launch_bounds__(1024) void sample_rays_kernel(const RayArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t step = a.counter ? *a.counter : a.offset;
    if (a.ep.images && a.bump) reshuffle_epoch(a.ep, a.seed, step);      // (a.bump: this is the single workgroup)
    if (i < a.batch) sample_ray(a, step, i);
    if (a.bump) {
        __syncthreads();
        if (threadIdx.x == 0) *a.bump = step + 1;
    }
}

__device__ __forceinline__ void sample_ray(const RayArgs& a, uint64_t step, int i) {
    int img = a.img_idx;
    if (img < 0) {
        if (a.ep.n > 0) img = a.ep.perm[step % (uint64_t)a.ep.n];
        else img = a.ds.image_perm ? a.ds.image_perm[step % (uint64_t)a.ds.n_images] : (int)(step % (uint64_t)a.ds.n_images);
    }
    const int H = a.ds.H, W = a.ds.W, HW = H * W;
    int px, py;
    uint32_t r[4];
    if (!a.pixels_in || a.out.t_rand) Philox::gen(a.seed, step, (uint64_t)i, r);
    // render()'s per-ray jitter torch.rand([N,1]) - 0.5 (udf_renderer_blending.py:719) from word 2 of the ray's draw: U(-0.5, 0.5) on a 2^-24 grid
    if (a.out.t_rand) a.out.t_rand[i] = (float)(r[2] >> 8) * (1.0f / 16777216.0f) - 0.5f;
    if (a.pixels_in) {
        px = (int)a.pixels_in[2 * i]; py = (int)a.pixels_in[2 * i + 1];
    } else {
        const int half = a.batch / 2;
        if (!a.importance || i < half) {                        // dataset.py:233-234 / 244-245
            px = rand_below(r[0], W); py = rand_below(r[1], H);
        } else {                                                // dataset.py:254-260
            const int ne = a.ds.n_edge[img], nn = HW - ne;
            const float d = a.ds.density[img];
            const double we = (double)ne * (1.0 - (double)d), wn = (double)nn * (double)d;
            const double u = ((double)r[0] + 0.5) * (1.0 / 4294967296.0) * (we + wn);
            const int32_t* order = a.ds.pixel_order + (size_t)img * HW;
            int pix;
            if ((u < we && ne > 0) || nn == 0) pix = order[rand_below(r[1], ne)];
            else pix = order[ne + rand_below(r[1], nn)];
            px = pix % W; py = pix / W;
        }
    }
    const float* K = a.ds.kinv + (size_t)img * 9;
    const float* P = a.ds.pose + (size_t)img * 16;
    const float fx = (float)px, fy = (float)py;
    // p = K^-1 [x, y, 1]   (dataset.py:272-277)
    const float p0 = K[0] * fx + K[1] * fy + K[2], p1 = K[3] * fx + K[4] * fy + K[5], p2 = K[6] * fx + K[7] * fy + K[8];
    const float n = sqrtf(p0 * p0 + p1 * p1 + p2 * p2);
    const float v0 = p0 / n, v1 = p1 / n, v2 = p2 / n;          // :279
    if (a.out.depth_scale) a.out.depth_scale[i] = v2;           // :280
    if (a.out.rays_v) {                                         // :281-283
        a.out.rays_v[3 * i + 0] = P[0] * v0 + P[1] * v1 + P[2] * v2;
        a.out.rays_v[3 * i + 1] = P[4] * v0 + P[5] * v1 + P[6] * v2;
        a.out.rays_v[3 * i + 2] = P[8] * v0 + P[9] * v1 + P[10] * v2;
    }
    if (a.out.rays_o) { a.out.rays_o[3 * i] = P[3]; a.out.rays_o[3 * i + 1] = P[7]; a.out.rays_o[3 * i + 2] = P[11]; }   // :284-286
    if (a.out.edge) a.out.edge[i] = a.ds.edges[(size_t)img * HW + (size_t)py * W + px];                                // :270
    if (a.out.ndc_uv) {                                         // :265-267
        a.out.ndc_uv[2 * i] = 2.0f * fx / (float)(W - 1) - 1.0f;
        a.out.ndc_uv[2 * i + 1] = 2.0f * fy / (float)(H - 1) - 1.0f;
    }
    if (a.out.p_cam) { a.out.p_cam[3 * i] = p0; a.out.p_cam[3 * i + 1] = p1; a.out.p_cam[3 * i + 2] = p2; }
    if (a.out.pixels) { a.out.pixels[2 * i] = px; a.out.pixels[2 * i + 1] = py; }
    if (a.out.img_idx && i == 0) a.out.img_idx[0] = img;
}

__global__ void bump_counter_kernel(uint64_t* c) { *c += 1; }

static int sample_rays(const EmapRayDataset* ds, const EpochArgs& ep, int img_idx, int batch, int importance, uint64_t seed, uint64_t offset,
                       uint64_t* counter, const int64_t* pixels_in, const EmapRayBatch* out, hipStream_t st) {
    if (!ds || !out) { set_error("sample_rays: null pointer"); return EMAP_E_INVALID; }
    if (!ds->edges || !ds->kinv || !ds->pose || ds->n_images < 1 || ds->H < 2 || ds->W < 2) { set_error("sample_rays: incomplete dataset"); return EMAP_E_INVALID; }
    if (img_idx >= ds->n_images) { set_error("sample_rays: image %d out of range", img_idx); return EMAP_E_INVALID; }
    if (importance && !pixels_in && (!ds->pixel_order || !ds->n_edge || !ds->density)) { set_error("sample_rays: importance sampling needs pixel_order / n_edge / density"); return EMAP_E_INVALID; }
    if (batch <= 0) return EMAP_OK;
    RayArgs a;
    a.ds = *ds; a.out = *out; a.ep = ep; a.pixels_in = pixels_in; a.counter = counter; a.seed = seed; a.offset = offset;
    a.img_idx = img_idx; a.batch = batch; a.importance = importance;
    const bool one_wg = batch <= 1024;
    a.bump = one_wg ? counter : nullptr;
    if (one_wg) hipLaunchKernelGGL(sample_rays_kernel, dim3(1), dim3((batch + 63) / 64 * 64), 0, st, a);
    else {
        if (ep.images) hipLaunchKernelGGL(reshuffle_epoch_kernel, dim3(1), dim3(1024), 0, st, ep, counter, seed);
        hipLaunchKernelGGL(sample_rays_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, a);
        if (counter) hipLaunchKernelGGL(bump_counter_kernel, dim3(1), dim3(1), 0, st, counter);
    }
    return check_launch("sample_rays");
}

int launch_sample_rays(const EmapRayDataset* ds, int img_idx, int batch, int importance, uint64_t seed, uint64_t offset,
                       uint64_t* counter, const int64_t* pixels_in, const EmapRayBatch* out, hipStream_t st) {
    return sample_rays(ds, EpochArgs{nullptr, nullptr, nullptr, 0}, img_idx, batch, importance, seed, offset, counter, pixels_in, out, st);
}

// ---- a training list with a new order every epoch (runner_udf.py:46, 249-250) ----
int check_train_images(const int32_t* images, int n_train, int n_images) {
    if (!images) { set_error("check_train_images: null list"); return EMAP_E_INVALID; }
    if (n_images < 1) { set_error("check_train_images: n_images must be >= 1 (got %d)", n_images); return EMAP_E_INVALID; }
    if (n_train <= 0) { set_error("check_train_images: the list is empty (n_train = %d)", n_train); return EMAP_E_INVALID; }
    if (n_train > EMAP_MAX_TRAIN_IMAGES) { set_error("check_train_images: %d images, at most %d", n_train, EMAP_MAX_TRAIN_IMAGES); return EMAP_E_INVALID; }
    for (int i = 0; i < n_train; ++i) {
        if (images[i] < 0 || images[i] >= n_images) { set_error("check_train_images: entry %d is image %d, outside [0, %d)", i, images[i], n_images); return EMAP_E_INVALID; }
        for (int j = 0; j < i; ++j)
            if (images[j] == images[i]) { set_error("check_train_images: image %d appears twice (entries %d and %d)", images[i], j, i); return EMAP_E_INVALID; }
    }
    return EMAP_OK;
}

int launch_sample_rays_train(const EmapRayDataset* ds, const int32_t* train_images, int n_train, int32_t* perm, int64_t* epoch_tag, int batch,
                             int importance, uint64_t seed, uint64_t* counter, const int64_t* pixels_in, const EmapRayBatch* out, hipStream_t st) {
    if (!ds || !out || !perm || !counter) { set_error("sample_rays_train: null pointer (ds, out, perm and counter_dev are required)"); return EMAP_E_INVALID; }
    if (train_images && !epoch_tag) { set_error("sample_rays_train: train_images without epoch_tag"); return EMAP_E_INVALID; }
    if (n_train <= 0) { set_error("sample_rays_train: n_train must be >= 1 (got %d)", n_train); return EMAP_E_INVALID; }
    if (n_train > EMAP_MAX_TRAIN_IMAGES || n_train > ds->n_images) {
        set_error("sample_rays_train: n_train %d above the limit (%d, and the %d images of the dataset)", n_train, EMAP_MAX_TRAIN_IMAGES, ds->n_images);
        return EMAP_E_INVALID;
    }
    return sample_rays(ds, EpochArgs{train_images, perm, epoch_tag, n_train}, -1, batch, importance, seed, 0, counter, pixels_in, out, st);
}

// ---- full-image rays: Dataset.gen_rays_at (dataset.py:137-167) ----------------------------------------------------------------------
// The rays of a whole validation view, from the K^-1 and poses the sampler already keeps on the device.  The reference builds a
// meshgrid over the image on the HOST, runs two batched 3x3 matmuls over its pixels and copies five tensors to the GPU; here one thread
// per ray writes rays [first, first + count) of the view in row-major (H/l, W/l) order - the order of the reference's TRANSPOSED
// rays_o / rays_v (:162-163) - so a caller renders a view chunk by chunk and the view's rays never exist in full.
// Pixel coordinates are torch.linspace(0, W-1, W//l) / linspace(0, H-1, H//l) (:142-143), non-integer for l > 1: ATen's formula, a step
// from the start for the first half and from the end for the second, each product and difference rounded on its own.
// The camera arithmetic is sample_ray's above, on those coordinates.  Bound: HBM writes, 28 B per ray; nothing is read but 25 floats.

__device__ __forceinline__ float view_coord(float last, int steps, int i) {
#pragma clang fp contract(off)
    if (steps == 1) return 0.0f;
    const float step = last / (float)(steps - 1);
    const float up = step * (float)i, down = step * (float)(steps - i - 1);
    return (i < steps / 2) ? up : last - down;
}

struct ViewArgs {
    const float* kinv;
    const float* pose;
    const int32_t* image_perm;
    float *rays_o, *rays_d, *depth_scale;
    long long first, count;
    int32_t img_idx, n_images, H, W, h, w;
};

__global__ __launch_bounds__(256) void gen_rays_at_kernel(const ViewArgs a) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.count) return;
    int img = a.img_idx;
    if (img < 0) {                                              // entry -1 - img_idx of the runner's image permutation
        const int k = (int)((-1LL - (long long)img) % a.n_images);
        img = a.image_perm ? a.image_perm[k] : k;
    }
    const long long i = a.first + t;
    const int iy = (int)(i / a.w), ix = (int)(i - (long long)iy * a.w);
    const float fx = view_coord((float)(a.W - 1), a.w, ix), fy = view_coord((float)(a.H - 1), a.h, iy);   // :142-143
    const float* K = a.kinv + (size_t)img * 9;
    const float* P = a.pose + (size_t)img * 16;
    // p = K^-1 [x, y, 1]   (:145-150)
    const float p0 = K[0] * fx + K[1] * fy + K[2], p1 = K[3] * fx + K[4] * fy + K[5], p2 = K[6] * fx + K[7] * fy + K[8];
    const float n = sqrtf(p0 * p0 + p1 * p1 + p2 * p2);
    const float v0 = p0 / n, v1 = p1 / n, v2 = p2 / n;          // :151
    a.depth_scale[t] = v2;                                      // :152
    float* d = a.rays_d + t * 3;                                // :153-155
    d[0] = P[0] * v0 + P[1] * v1 + P[2] * v2;
    d[1] = P[4] * v0 + P[5] * v1 + P[6] * v2;
    d[2] = P[8] * v0 + P[9] * v1 + P[10] * v2;
    float* o = a.rays_o + t * 3;                                // :156-158
    o[0] = P[3]; o[1] = P[7]; o[2] = P[11];
}

int gen_rays_count(const EmapRayDataset* ds, int resolution_level, int64_t* n, int* h, int* w) {
    if (!ds) { set_error("gen_rays_count: null dataset"); return EMAP_E_INVALID; }
    if (ds->H < 1 || ds->W < 1) { set_error("gen_rays_count: image size %d x %d", ds->W, ds->H); return EMAP_E_INVALID; }
    if (resolution_level < 1) { set_error("gen_rays_count: resolution_level must be >= 1 (got %d)", resolution_level); return EMAP_E_INVALID; }
    const int hh = ds->H / resolution_level, ww = ds->W / resolution_level;
    if (hh == 0 || ww == 0) { set_error("gen_rays_count: resolution_level %d leaves no pixel of a %d x %d image", resolution_level, ds->W, ds->H); return EMAP_E_INVALID; }
    if (n) *n = (int64_t)hh * ww;
    if (h) *h = hh;
    if (w) *w = ww;
    return EMAP_OK;
}

int launch_gen_rays_at(const EmapRayDataset* ds, int img_idx, int resolution_level, int64_t first, int64_t count, float* rays_o, float* rays_d,
                       float* depth_scale, hipStream_t st) {
    int64_t total = 0;
    ViewArgs a;
    if (int rc = gen_rays_count(ds, resolution_level, &total, &a.h, &a.w)) return rc;
    if (!ds->kinv || !ds->pose || ds->n_images < 1) { set_error("gen_rays_at: incomplete dataset"); return EMAP_E_INVALID; }
    if (img_idx >= ds->n_images) { set_error("gen_rays_at: image %d out of range (%d images)", img_idx, ds->n_images); return EMAP_E_INVALID; }
    if (first < 0 || count < 0) { set_error("gen_rays_at: negative first / count"); return EMAP_E_INVALID; }
    if (count > total - first) { set_error("gen_rays_at: [first, first + count) leaves the view's %lld rays", (long long)total); return EMAP_E_INVALID; }
    if (count == 0) return EMAP_OK;
    if (!rays_o || !rays_d || !depth_scale) { set_error("gen_rays_at: null pointer"); return EMAP_E_INVALID; }
    a.kinv = ds->kinv; a.pose = ds->pose; a.image_perm = ds->image_perm; a.rays_o = rays_o; a.rays_d = rays_d; a.depth_scale = depth_scale;
    a.first = first; a.count = count; a.img_idx = img_idx; a.n_images = ds->n_images; a.H = ds->H; a.W = ds->W;
    hipLaunchKernelGGL(gen_rays_at_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, a);
    return check_launch("gen_rays_at");
}

}  // namespace emap
