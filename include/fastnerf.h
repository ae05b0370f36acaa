/* fastnerf.h -- C ABI of the MI355X-native NeRF training inner loop.
 *
 * Drop-in boundary for the renderer / quadtree path of
 * wen-yuan-zhang/Fast-Learning-NeRF (nerf-ours).  The reference has no FFI: the
 * path sits behind Python functions.  Every entry point below names the
 * reference function (file:line, relative to nerf-ours/) whose work it
 * replaces; INTEGRATION.md shows the ctypes stub a maintainer adds to call it.
 *
 * Conventions
 *   - all `float*`/`int*` arguments are DEVICE pointers unless the name ends in
 *     `_host`; buffers are owned by the caller (PyTorch's allocator); nothing
 *     is retained past return.
 *   - fp32, contiguous row-major.  rays are [N,11] = o(3) d(3) near far
 *     viewdir(3) (render.py:74-80).
 *   - every call enqueues work on `stream` (a hipStream_t) and returns without
 *     synchronising.
 *   - return 0 on success, <0 on error (-1 bad argument, -2 HIP error);
 *     fastnerf_last_error() returns a thread-local message.  Never aborts.
 */
#ifndef FASTNERF_H
#define FASTNERF_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* fn_stream_t; /* hipStream_t */

int fastnerf_version(void);
const char* fastnerf_last_error(void);
/* device properties used by bench/tests: returns CU count (or <0) */
int fastnerf_device_cus(void);
/* paired dW trunk launches (one launch for the trunk jobs of both passes of a bf16x6 step) this process has enqueued so far:
 * tells which route a backward took; the unpaired route computes the same gradients */
int64_t fastnerf_x6_pair_launches(void);
/* backward passes this process has enqueued whose view-layer dW job REBUILT dYv (the gradient at the view layer's pre-activation) on chip from
 * hv, d(loss)/d(raw) and the rgb weights instead of reading it: the backward phases of fastnerf_train_step* in bf16x6 on the plain backward.
 * dX then does not store dYv: after such a step the dYv region of dact_ws (the last 128 floats a point) holds nothing.  FASTNERF_SIDE_REBUILD=0
 * in the environment, read at every call, selects the reading route with the store on; =nan fills the region with NaNs first.  The gradients
 * are bit-identical on both routes.  Every other entry point stores and reads dYv as before. */
int64_t fastnerf_side_rebuild_passes(void);

/* ---- rays ------------------------------------------------------------- */
/* get_rays (run_nerf_helpers.py:68-78): all H*W pixels of one camera.
 * c2w_host: 12 floats (3x4 row-major).  rays_o/rays_d: [H,W,3]. */
int fastnerf_gen_rays(int H, int W, float fx, float fy, float cx, float cy, const float* c2w_host,
                      float* rays_o, float* rays_d, fn_stream_t stream);
/* rays for selected pixels of many cameras (tree.py:617-619 gather restated as
 * on-the-fly generation): pix [n,3] int32 (image, row, col); poses [n_img,3,4]. */
int fastnerf_gen_rays_pixels(int64_t n, const int32_t* pix, const float* poses, float fx, float fy, float cx,
                             float cy, float* rays_o, float* rays_d, fn_stream_t stream);
/* ndc_rays (run_nerf_helpers.py:91-108), in -> out [n,3] each. */
int fastnerf_ndc_rays(int64_t n, int H, int W, double focal, float near, const float* rays_o, const float* rays_d,
                      float* out_o, float* out_d, fn_stream_t stream);
/* render() prologue (render.py:59-80): viewdirs = d/|d| (before ndc), optional
 * ndc warp, pack [n,11]. */
int fastnerf_pack_rays(int64_t n, const float* rays_o, const float* rays_d, float near, float far, int ndc, int H,
                       int W, double focal, float* rays11, fn_stream_t stream);
/* coarse depths (render.py:244-266).  t_rand: [n,S] injected U[0,1) jitter, or
 * NULL; when NULL and perturb!=0 a Philox stream keyed by (seed, ray, sample)
 * is used.  z: [n,S]. */
int fastnerf_sample_coarse(int64_t n, int S, const float* rays11, int lindisp, int perturb, const float* t_rand,
                           uint64_t seed, float* z, fn_stream_t stream);
/* Embedder.embed (run_nerf_helpers.py:15-63): x [n,3] -> out [n, 3+6L]. */
int fastnerf_posenc(int64_t n, int L, const float* x, float* out, fn_stream_t stream);

/* ---- MLP (model.py:8-63, D=8 W=256 skip@4 use_viewdirs) ---------------- */
#define FASTNERF_NET_PARAMS 595844      /* floats per net, model.parameters() order */
#define FASTNERF_PACKED_FWD 663680      /* floats: fragment-ordered forward weights (kind 0; in general fastnerf_net_floats(kind, 1)) */
#define FASTNERF_PACKED_BWD 589824      /* floats: fragment-ordered transposed weights (fastnerf_net_floats(kind, 2)) */
/* saved activations: n*S*FASTNERF_ACT_FLOATS + FASTNERF_ACT_SLACK floats
 * (per point pe64 + 8*h256 + feat256 + vpe32 + hv128 + 64 floats of ReLU sign words) */
#define FASTNERF_ACT_FLOATS 2592
#define FASTNERF_ACT_SLACK 8192   /* kind 0; in general use fastnerf_mlp_act_floats() */
/* per-point pre-activation gradients (floats): 8*dY256 + dfeat256 + dYv128 */
#define FASTNERF_DACT_FLOATS 2432

/* re-layout of one net's flat parameters into the MFMA fragment order used by
 * mlp_fwd (packed_fwd) and mlp_bwd_dx (packed_bwd). */
int fastnerf_mlp_pack(const float* params, float* packed_fwd, float* packed_bwd, fn_stream_t stream);
/* run_network (run_nerf.py:50-64) + NeRF.forward: points are generated on the
 * fly from rays11 [n,11] and z [n,S] (pts = o + d*z, render.py:268), encoded
 * (L=10 / L=4) and pushed through the MLP.  raw: [n,S,4] (rgb logits, sigma).
 * act: NULL (inference) or a buffer of n*S*FASTNERF_ACT_FLOATS + FASTNERF_ACT_SLACK floats that
 * receives the activations backward needs. */
int fastnerf_mlp_fwd(int64_t n, int S, const float* rays11, const float* z, const float* params,
                     const float* packed_fwd, float* raw, float* act, fn_stream_t stream);
/* backward of the above w.r.t. the parameters: draw [n,S,4] -> grads (same
 * layout as params, OVERWRITTEN).  dact: scratch n*S*FASTNERF_DACT_FLOATS;
 * partial: scratch of fastnerf_mlp_bwd_partial_floats() floats. */
int64_t fastnerf_mlp_bwd_partial_floats(void);
int fastnerf_mlp_bwd(int64_t n, int S, const float* draw, const float* act, const float* params,
                     const float* packed_bwd, float* dact, float* partial, float* grads, fn_stream_t stream);

/* ---- compositing / hierarchical sampling ------------------------------ */
/* raw2outputs (render.py:149-192).  noise: [n,S] scaled sigma noise or NULL.
 * outputs: rgb_map [n,3], disp [n], acc [n], weights [n,S], depth [n]. */
int fastnerf_raw2outputs_fwd(int64_t n, int S, const float* raw, const float* z, const float* rays11,
                             const float* noise, int white_bkgd, float* rgb_map, float* disp, float* acc,
                             float* weights, float* depth, fn_stream_t stream);
/* d(rgb_map)/d(raw): g_rgb [n,3] -> draw [n,S,4]. */
int fastnerf_raw2outputs_bwd(int64_t n, int S, const float* raw, const float* z, const float* rays11,
                             const float* noise, int white_bkgd, const float* g_rgb, float* draw,
                             fn_stream_t stream);
/* d(rgb_map, disp, acc, weights, depth)/d(raw) (render.py:149-192, every output differentiable as in the
 * reference's autograd): upstream g_rgb [n,3], g_disp [n], g_acc [n], g_w [n,S], g_depth [n], each NULL = zero.
 * acc / depth: the forward's outputs (needed when g_disp != NULL: they decide the disparity clamp and its NaN
 * branch).  -> draw [n,S,4].  With only g_rgb given, bit-identical to fastnerf_raw2outputs_bwd. */
int fastnerf_raw2outputs_bwd_full(int64_t n, int S, const float* raw, const float* z, const float* rays11,
                                  const float* noise, int white_bkgd, const float* acc, const float* depth,
                                  const float* g_rgb, const float* g_disp, const float* g_acc, const float* g_w,
                                  const float* g_depth, float* draw, fn_stream_t stream);
/* sample_pdf (run_nerf_helpers.py:112-155) on bins = mid(z), weights[1:-1],
 * followed by sort(cat[z, z_samples]) (render.py:279-283).  u: [n,Ni] injected
 * uniforms or NULL; det!=0 -> linspace(0,1,Ni); else Philox(seed).
 * z_out: [n,S+Ni] sorted; z_samples: [n,Ni] (may be NULL); z_std [n] (may be NULL). */
int fastnerf_sample_pdf_merge(int64_t n, int S, int Ni, const float* z, const float* weights, int det,
                              const float* u, uint64_t seed, float* z_out, float* z_samples, float* z_std,
                              fn_stream_t stream);

/* stand-alone sample_pdf(bins [n,M], weights [n,M-1]) -> samples [n,Ni]
 * (run_nerf_helpers.py:112-155 as called by third parties, e.g. tests). */
int fastnerf_sample_pdf(int64_t n, int M, int Ni, const float* bins, const float* weights, int det, const float* u,
                        uint64_t seed, float* samples, fn_stream_t stream);

/* ---- loss / optimiser / quadtree loss map ------------------------------ */
/* img2mse (run_nerf_helpers.py:9) for fine and coarse maps + their gradients
 * + the per-(image, leaf) max |gt - pred| table (tree.py:538, 632-642).
 * loss2: 2 floats (fine mse, coarse mse), accumulated from zero by the call.
 * leaf_tag: [n,2] int32 (image, leaf) or NULL; table: [n_img*max_leaves] uint32
 * bit patterns of non-negative floats (atomicMax), or NULL.
 * grad_scale multiplies 2/(3n) (data-parallel: n_local/n_global). */
int fastnerf_mse_leafmax(int64_t n, const float* rgb, const float* rgb0, const float* target, float grad_scale,
                         float* g_rgb, float* g_rgb0, float* loss2, const int32_t* leaf_tag, int max_leaves,
                         uint32_t* table, fn_stream_t stream);
/* Auxiliary losses on the depth and opacity maps of render_rays (render.py:149-192 hands out depth_map / acc_map, and the
 * reference's loss of run_nerf.py:479-494 is plain torch, so any term on them trains both networks).  Per pass p (1 = the
 * pass that produces the image, 0 = the coarse pass of a two-pass render; depth0 / acc0 / g_depth0 / g_acc0 NULL with one pass):
 *   Ld_p = 1/n sum_r wd_r (depth_p[r] - D_r)^2     g_depth_p[r] = grad_scale lambda_depth 2 wd_r (depth_p[r] - D_r) / n
 *   La_p = 1/n sum_r wa_r (acc_p[r]   - A_r)^2     g_acc_p[r]   = grad_scale lambda_acc   2 wa_r (acc_p[r]   - A_r) / n
 * loss4 = (Ld_1, Ld_0, La_1, La_0), unscaled by the lambdas, WRITTEN (not accumulated) by the call.  A NULL weight means ones;
 * a NULL target switches its term off (losses 0, its gradient buffers untouched).  A ray whose weight is 0 contributes exactly 0
 * and gets a gradient of exactly +0 whatever its target holds (sparse depth: NaN where unknown, weight 0).  One workgroup sums
 * in a fixed order in fp64 and no atomics are used: two calls on the same input are bit-identical, for every n. */
int fastnerf_aux_loss(int64_t n, const float* depth1, const float* acc1, const float* depth0, const float* acc0,
                      const float* depth_target, const float* depth_weight, const float* acc_target, const float* acc_weight,
                      float lambda_depth, float lambda_acc, float grad_scale, float* g_depth1, float* g_acc1, float* g_depth0,
                      float* g_acc0, float* loss4, fn_stream_t stream);
/* torch.optim.Adam step (run_nerf.py:99,494) over a flat buffer.  params, grads, m and v are read as float4: each must be 16-byte
 * aligned (a slice of a flat buffer starts at a multiple of four floats), else the call returns an error and launches nothing; n
 * itself may be any positive count. */
int fastnerf_adam_step(int64_t n, float* params, const float* grads, float* m, float* v, double lr, double beta1,
                       double beta2, double eps, int step, fn_stream_t stream);

/* ---- generalised MLP entry points: kind 0 = NeRF (model.py), 1 = nerf++ MLPNet foreground,
 * 2 = nerf++ MLPNet background (4-D inverted-sphere input, samples consumed far->near;
 * nerf++-ours/nerf_network.py:70-142, ddp_model.py:110-124) ------------------------------------- */
/* what: 0 parameter floats, 1 packed-forward floats, 2 packed-backward floats, 3 padded PE width */
int64_t fastnerf_net_floats(int kind, int what);
int64_t fastnerf_mlp_act_floats(int kind, int64_t n_points);
int fastnerf_mlp_pack_ex(int kind, const float* params, float* packed_fwd, float* packed_bwd, fn_stream_t stream);
int fastnerf_mlp_fwd_ex(int kind, int64_t n, int S, const float* rays11, const float* z, const float* params,
                        const float* packed_fwd, float* raw, float* act, fn_stream_t stream);
int fastnerf_mlp_bwd_ex(int kind, int64_t n, int S, const float* draw, const float* act, const float* params,
                        const float* packed_bwd, float* dact, float* partial, float* grads, fn_stream_t stream);

/* ---- split-bf16 ("bf16x3") math mode, all three net kinds ------------------------------------------
 * Same network functions and call protocol as fastnerf_mlp_pack_ex / fwd_ex / bwd_ex (run_nerf.py:91-107
 * run_network -> model.py:37-63, autograd backward of the same), computed on the bf16 matrix cores: every fp32
 * operand is carried as a (hi, lo) bf16 pair and products are hi*hi + hi*lo + lo*hi with fp32 accumulation
 * (csrc/mlp_bf16.hip).  Buffers are opaque and sized by fastnerf_mlp_bf16_floats (in 4-byte units):
 * what 1 packed forward weights, 2 packed backward weights, 3 saved activations for n_points, 4 pre-activation
 * gradients for n_points.  act == NULL in fwd: inference, nothing saved. */
int64_t fastnerf_mlp_bf16_floats(int kind, int what, int64_t n_points);
int64_t fastnerf_mlp_bf16_partial_floats(void);
int fastnerf_mlp_bf16_pack(int kind, const float* params, float* packed_fwd, float* packed_bwd, fn_stream_t stream);
int fastnerf_mlp_bf16_fwd(int kind, int64_t n, int S, const float* rays11, const float* z, const float* params,
                          const float* packed_fwd, float* raw, float* act, fn_stream_t stream);
int fastnerf_mlp_bf16_bwd(int kind, int64_t n, int S, const float* draw, const float* act, const float* params,
                          const float* packed_bwd, float* dact, float* partial, float* grads, fn_stream_t stream);

/* Inference forward (no saved activations) with options.  flags & FN_FWD_SKIP_DEAD_RGB (kind 0 only): a
 * 64-point tile whose samples ALL have sigma <= 0 skips the feature layer, the view layer and the colour head and reports
 * colour logits 0 -- valid when nothing reads the colour of a sample whose weight is exactly zero: compositing without sigma
 * noise (render.py:162-182: alpha = 1 - exp(-relu(sigma) * dist) = 0, weight = alpha * T = 0) and everything downstream of it
 * (rgb / disp / acc maps, inverse-CDF weights, every gradient).  The sigma channel is always exact. */
#define FN_FWD_SKIP_DEAD_RGB 1
int fastnerf_mlp_bf16_fwd_flags(int kind, int64_t n, int S, const float* rays11, const float* z, const float* params,
                                const float* packed_fwd, float* raw, int flags, fn_stream_t stream);
int fastnerf_mlp_fwd_flags_ex(int kind, int64_t n, int S, const float* rays11, const float* z, const float* params,
                              const float* packed_fwd, float* raw, int flags, fn_stream_t stream);   /* exact-fp32 kernels */

/* ---- fused forward of render_rays (render.py:238-299): coarse sampler -> coarse MLP -> compositing ->
 * [sample_pdf + merge -> fine MLP -> compositing], enqueued by one call on `stream`.  math_mode 0 = exact fp32,
 * 1 = split-bf16 (x3), 2 = bf16x6; packed_* must come from the matching pack entry point; act0 / act1 == NULL: inference.  perturb /
 * t_rand / seed0 as fastnerf_sample_coarse, det / u / seed1 as fastnerf_sample_pdf_merge, noise* as
 * fastnerf_raw2outputs_fwd.  N_importance == 0: coarse pass only (the *_f / *1 arguments are ignored).  All buffers
 * are caller-owned device memory with the shapes of the individual entry points. */
int fastnerf_render_rays_fwd(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11, int lindisp,
                             int perturb, int det, int white_bkgd, const float* t_rand, const float* u,
                             const float* noise0, const float* noise1, uint64_t seed0, uint64_t seed1,
                             const float* params_c, const float* packed_c, const float* params_f, const float* packed_f,
                             float* z0, float* raw0, float* act0, float* rgb0, float* disp0, float* acc0, float* w0,
                             float* depth0, float* z1, float* z_samples, float* z_std, float* raw1, float* act1,
                             float* rgb1, float* disp1, float* acc1, float* w1, float* depth1, fn_stream_t stream);
/* The same with fastnerf_mlp_bf16_fwd_flags options for its inference launches (act0 / act1 == NULL, noise0 / noise1 == NULL;
 * ignored otherwise): what the first pass of a compacted training step uses -- raw0 / raw1 then carry colour
 * logits 0 on tiles without a live sample, every other output is bit-identical. */
int fastnerf_render_rays_fwd_ex(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11, int lindisp,
                                int perturb, int det, int white_bkgd, const float* t_rand, const float* u,
                                const float* noise0, const float* noise1, uint64_t seed0, uint64_t seed1,
                                const float* params_c, const float* packed_c, const float* params_f, const float* packed_f,
                                float* z0, float* raw0, float* act0, float* rgb0, float* disp0, float* acc0, float* w0,
                                float* depth0, float* z1, float* z_samples, float* z_std, float* raw1, float* act1,
                                float* rgb1, float* disp1, float* acc1, float* w1, float* depth1, int flags, fn_stream_t stream);

/* Backward of the same chain w.r.t. the network parameters (what loss.backward() does for this path,
 * run_nerf.py:493): fine pass into grads_f, coarse pass into grads_c (sample positions are detached, so the coarse net
 * only sees g_rgb0).  Two distinct nets when N_importance > 0.  draw_ws: n*(N_samples+N_importance)*4 floats;
 * dact_ws / partial_ws as for the mlp_bwd entry points. */
int fastnerf_render_rays_bwd(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11, int white_bkgd,
                             const float* g_rgb, const float* g_rgb0, const float* noise0, const float* noise1,
                             const float* z0, const float* raw0, const float* act0, const float* z1, const float* raw1,
                             const float* act1, const float* params_c, const float* packed_bwd_c, const float* params_f,
                             const float* packed_bwd_f, float* draw_ws, float* dact_ws, float* partial_ws, float* grads_c,
                             float* grads_f, fn_stream_t stream);

/* ---- nerf++-ours additions ------------------------------------------- */
/* get_rays_single_image (nerf_sample_ray_split.py:10-34): intrinsics_host / c2w_host are 4x4 row-major
 * doubles; rays_o / rays_d [H*W,3]. */
int fastnerf_pp_gen_rays(int H, int W, const double* intrinsics_host, const double* c2w_host, float* rays_o,
                         float* rays_d, fn_stream_t stream);
/* nerf++ quadtree fork: per-(image, leaf) sum of |gt-pred| over rays and channels (fp64) and ray count
 * feeding the MEAN split criterion (nerf++-ours/tree.py:622); the caller zeroes sum / count.  A ray's term is rounded to a
 * multiple of 2^-30 before it is added: the sums are exact (< 2^23), order independent and shard independent. */
int fastnerf_leaf_sumcount(int64_t n, const float* rgb, const float* target, const int32_t* leaf_tag, int max_leaves,
                           double* sum, int32_t* count, fn_stream_t stream);
/* intersect_sphere (ddp_train_nerf.py:54-69); *n_outside counts rays whose camera is not inside the
 * unit sphere (the reference raises in that case). */
int fastnerf_pp_intersect_sphere(int64_t n, const float* rays11, float* fg_far, int* n_outside, fn_stream_t stream);
/* foreground depths near + i*step, optionally perturbed (ddp_train_nerf.py:355-361, 72-81). */
int fastnerf_pp_fg_depths(int64_t n, int S, float near, const float* fg_far, int perturb, const float* t_rand,
                          uint64_t seed, float* z, fn_stream_t stream);
/* nerf++ sample_pdf + sort-merge (ddp_train_nerf.py:84-133, 369-382). */
int fastnerf_pp_sample_pdf_merge(int64_t n, int S, int Ni, const float* z, const float* weights, int det,
                                 const float* u, uint64_t seed, float* z_out, float* z_samples, fn_stream_t stream);
/* perturb_samples (ddp_train_nerf.py:72-81): z_out = lower + (upper - lower) * u over the mid-point intervals of the sorted
 * depths z_in [n,S]; t_rand [n,S] injected or NULL (Philox(seed)).  z_out must not alias z_in. */
int fastnerf_pp_perturb_samples(int64_t n, int S, const float* z_in, const float* t_rand, uint64_t seed, float* z_out,
                                fn_stream_t stream);
/* stand-alone nerf++ sample_pdf (ddp_train_nerf.py:84-133): bins [n,M], weights [n,M-1] -> samples [n,Ni]. */
int fastnerf_pp_sample_pdf(int64_t n, int M, int Ni, const float* bins, const float* weights, int det, const float* u,
                           uint64_t seed, float* samples, fn_stream_t stream);
/* depth2pts_outside (ddp_model.py:16-45): ray_o / ray_d [n,3], depth [n,S] (inverse distance to the sphere origin) ->
 * pts [n,S,4] = (x', y', z', 1/r), depth_real [n,S] (may be NULL). */
int fastnerf_pp_depth2pts_outside(int64_t n, int S, const float* ray_o, const float* ray_d, const float* depth, float* pts,
                                  float* depth_real, fn_stream_t stream);
/* fg (part 0) / bg (part 1) compositing of NerfNet.forward (ddp_model.py:97-135) and its backward.
 * raw is the MLP output in network order (bg: far->near); z is always stored near->far.
 * fwd outputs: rgb_map [n,3], weights [n,S], depth [n] (may be NULL), lambda [n] (part 0 only).
 * bwd inputs: g_rgb [n,3], g_lambda [n] (part 0; may be NULL) -> draw [n,S,4]. */
int fastnerf_pp_composite_fwd(int64_t n, int S, int part, const float* raw, const float* z, const float* rays11,
                              const float* fg_far, float* rgb_map, float* weights, float* depth, float* lambda,
                              fn_stream_t stream);
int fastnerf_pp_composite_bwd(int64_t n, int S, int part, const float* raw, const float* z, const float* rays11,
                              const float* fg_far, const float* g_rgb, const float* g_lambda, float* draw,
                              fn_stream_t stream);

/* ---- host quadtree (tree.py), no device work --------------------------- */
typedef struct fn_tree fn_tree; /* opaque: per-image DFS leaf lists */
fn_tree* fastnerf_tree_create(int H, int W, int n_images, int max_depth);
void fastnerf_tree_destroy(fn_tree* t);
int fastnerf_tree_num_leaves(const fn_tree* t, int image);
int fastnerf_tree_max_leaves(const fn_tree* t);
double fastnerf_tree_min_area(const fn_tree* t, int image);
/* leaves of one image in DFS enumeration order: out [n_leaves,4] doubles x0,y0,x1,y1 */
int fastnerf_tree_get_leaves(const fn_tree* t, int image, double* out_host);
int fastnerf_tree_set_leaves(fn_tree* t, int image, int n_leaves, const double* boxes_host, double min_area);
/* per-leaf ray count + integer pixel ranges (tree.py:578-581, 598-599):
 * out [n_leaves,5] int32: count, row_lo, row_hi, col_lo, col_hi (hi exclusive).
 * last_epoch!=0 evaluates a fresh depth-1 tree (tree.py:390-400). */
int fastnerf_tree_leaf_plan(const fn_tree* t, int image, double ray_num_per_pixel, int last_epoch,
                            int32_t* out_host);
/* adjust_tree_multiThread (tree.py:533-557, 629-652) driven by the reduced
 * table: table_host [n_images, max_leaves] floats (max |gt-pred| per leaf,
 * negative = leaf had no ray).  Returns total leaves after the split, <0 on error. */
int64_t fastnerf_tree_adjust(fn_tree* t, const float* table_host, int max_leaves, double thres);
/* nerf++ fork: mean criterion from fp64 sums + counts ([n_images, max_leaves] each). */
int64_t fastnerf_tree_adjust_mean(fn_tree* t, const double* sum_host, const int32_t* count_host, int max_leaves,
                                  double thres);


/* ---- epoch ray generation on the device (gen_rays_v3_multiThread + gen_rays_v3_1_subThread, tree.py:377-428, 569-626;
 * the variance-weighted picks of nerf++-ours/tree.py:566-578 + image_process.py:58-93) ------------------------------
 * fastnerf_tree_epoch_plan (host): the plans of all trees in one call, rows of 7 int32 = image, leaf, ray count,
 * row_lo, row_hi, col_lo, col_hi; out_host may be NULL to query sizes; returns rows, *n_rays_host = total rays.
 * fastnerf_epoch_rays (device): N rows (rays_o, rays_d, rgb [N,3], tag [N,2] = image, leaf; pix [N,3] optional) in
 * their final shuffled order (replaces the per-leaf torch.randint draws, the [n,H,W,3] gathers and the epoch's
 * torch.randperm).  plan [L,7] and offs [L+1] (int64 exclusive prefix sums of the counts) are device copies of the
 * host plan; images [n_img,H,W,3], poses [n_img,3,4].  Weighted picks (all five pointers or none): per leaf the first
 * n_weighted[l] rays are drawn with probability proportional to the weights whose running sum over the pixels sorted
 * by leaf is cum (fp64); order = flat pixel ids in that order; seg_beg / seg_end = the leaf's range in it. */
int64_t fastnerf_tree_epoch_plan(const fn_tree* t, double ray_num_per_pixel, int last_epoch, int32_t* out_host,
                                 int64_t* n_rays_host);
int fastnerf_epoch_rays(int64_t N, int L, const int32_t* plan, const int64_t* offs, const float* images,
                        const float* poses, int n_img, int H, int W, float fx, float fy, float cx, float cy,
                        uint64_t seed, int shuffle, const int32_t* n_weighted, const int64_t* seg_beg,
                        const int64_t* seg_end, const int32_t* order, const double* cum, float* rays_o, float* rays_d,
                        float* rgb, int32_t* tag, int32_t* pix, fn_stream_t stream);
/* One rank's rows of the same epoch (data parallel): the reference cuts the shuffled epoch into batches of `batch` = N_rand
 * consecutive rows (run_nerf.py:472-478); rank row0 of `stride` ranks steps rows row0 :: stride of every batch.  Only those rows are
 * generated -- output row r = epoch row (r / per) * batch + row0 + (r % per) * stride, per = ceil((batch - row0) / stride) -- bit-identical to
 * the corresponding rows of fastnerf_epoch_rays with the same seed (the row -> ray map is a keyed bijection of the row index).
 * fastnerf_epoch_shard_rows: the number of output rows (host arithmetic; -1 on bad arguments). */
int64_t fastnerf_epoch_shard_rows(int64_t N, int64_t batch, int row0, int stride);
int fastnerf_epoch_rays_shard(int64_t N, int L, const int32_t* plan, const int64_t* offs, const float* images,
                              const float* poses, int n_img, int H, int W, float fx, float fy, float cx, float cy,
                              uint64_t seed, int shuffle, const int32_t* n_weighted, const int64_t* seg_beg,
                              const int64_t* seg_end, const int32_t* order, const double* cum, int64_t batch, int row0, int stride,
                              float* rays_o, float* rays_d, float* rgb, int32_t* tag, int32_t* pix, fn_stream_t stream);

/* sigma noise (render.py:162, `torch.randn(raw[..., 3].shape) * raw_noise_std`): out[0..n) = N(0, std^2) draws of a Philox4x32-10 stream keyed
 * by seed (Box-Muller), one launch for the noise of both passes of a render_rays call.  out must be 16-byte aligned. */
int fastnerf_gauss_noise(int64_t n, float std, uint64_t seed, float* out, fn_stream_t stream);

/* ---- exact zero-gradient point compaction of the training backward -------------------------------------------
 * loss.backward() (run_nerf.py:493) spends most of its time on samples whose d(loss)/d(raw) is exactly zero
 * (sigma + noise <= 0 => alpha = 0 => weight = 0 and relu' = 0; render.py:162,182): all of their pre-activation
 * gradients are exact zeros.  These entry points run the backward on the other ("live") samples only.
 * fastnerf_compact_live: live_idx[0..count) = ascending indices of the points p with draw[p*4..p*4+3] != 0,
 * count_out[0] = count, count_out[1] = n_points (device values: no host round trip).  ws: fastnerf_compact_ws_ints()
 * int32 of scratch. */
int64_t fastnerf_compact_ws_ints(int64_t n_points);
int fastnerf_compact_live(int64_t n_points, const float* draw, int32_t* live_idx, int32_t* count_out, int32_t* ws,
                          fn_stream_t stream);
/* NeRF.forward + Embedder.embed (model.py:38-63) over a live list, saving activations for the backward in list
 * order; act sized by fastnerf_mlp_bf16_floats(kind, 3, n*S). */
int fastnerf_mlp_bf16_fwd_live(int kind, int64_t n, int S, const float* rays11, const float* z, const float* params,
                               const float* packed_fwd, float* act, const int32_t* live_idx, const int32_t* live_cnt,
                               fn_stream_t stream);
/* backward of the MLP over the same list: draw is the full [n*S,4] gradient, read through live_idx. */
int fastnerf_mlp_bf16_bwd_live(int kind, int64_t n, int S, const float* draw, const float* act, const float* params,
                               const float* packed_bwd, float* dact, float* partial, float* grads,
                               const int32_t* live_idx, const int32_t* live_cnt, fn_stream_t stream);
/* the exact-fp32 twins (v_mfma_f32_32x32x2_f32 kernels; act sized by fastnerf_mlp_act_floats) */
int fastnerf_mlp_fwd_live_ex(int kind, int64_t n, int S, const float* rays11, const float* z, const float* params,
                             const float* packed_fwd, float* act, const int32_t* live_idx, const int32_t* live_cnt,
                             fn_stream_t stream);
int fastnerf_mlp_bwd_live_ex(int kind, int64_t n, int S, const float* draw, const float* act, const float* params,
                             const float* packed_bwd, float* dact, float* partial, float* grads,
                             const int32_t* live_idx, const int32_t* live_cnt, fn_stream_t stream);
/* the whole backward of render_rays (render.py:238-299 under loss.backward()) with compaction, for a forward that
 * saved nothing: per pass compositing backward -> live list -> saving forward over the list -> dX / dW
 * (math_mode 1: split-bf16, 0: exact fp32).
 * live_ws: 4 + n*(N_samples+N_importance) + fastnerf_compact_ws_ints(...) int32; counts_out: NULL or 4 int32
 * (live, total of the fine pass; live, total of the coarse pass). */
int fastnerf_render_rays_bwd_live(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11, int white_bkgd,
                                  const float* g_rgb, const float* g_rgb0, const float* noise0, const float* noise1,
                                  const float* z0, const float* raw0, const float* z1, const float* raw1,
                                  const float* params_c, const float* packed_fwd_c, const float* packed_bwd_c,
                                  const float* params_f, const float* packed_fwd_f, const float* packed_bwd_f,
                                  float* draw_ws, float* act_ws, float* dact_ws, float* partial_ws, int32_t* live_ws,
                                  float* grads_c, float* grads_f, int32_t* counts_out, fn_stream_t stream);

/* ---- every rendered map differentiable on the fused route (render.py:149-192: disp_map, acc_map, depth_map and their coarse
 * twins are plain torch in the reference, so a loss on them reaches both networks; run_nerf.py:479-494) ------------------------
 * fn_map_grads: d(loss)/d(disp, acc, depth) of the fine pass (1) and of the coarse pass (0), [n] each, each NULL = zero.  With
 * N_importance == 0 the *1 members belong to the only pass, as g_rgb does.  The _maps entry points are the plain ones plus the
 * forward's acc0, depth0, acc1, depth1 (the disparity clamp and its NaN branch are decided on them; needed where a g_disp is set)
 * and the struct (NULL = no map gradient).  A pass none of whose three members is set makes exactly the plain entry point's
 * fastnerf_raw2outputs_bwd call (the plain entry points are that case); a pass with one set calls fastnerf_raw2outputs_bwd_full,
 * and its g_rgb may then be NULL.  A sample with sigma' <= 0 still has draw == +-0 in all four components (w = alpha T = 0 and the
 * density term is gated by sigma' > 0), so the live list of the compacted route stays exact -- but an opacity or depth term makes
 * every sample with sigma' > 0 of a ray that has not saturated live, where the colour loss alone left the occluded ones dead. */
typedef struct fn_map_grads {
  const float *g_disp1, *g_acc1, *g_depth1, *g_disp0, *g_acc0, *g_depth0;
} fn_map_grads;
int fastnerf_render_rays_bwd_maps(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11, int white_bkgd,
                                  const float* g_rgb, const float* g_rgb0, const float* noise0, const float* noise1,
                                  const float* z0, const float* raw0, const float* act0, const float* z1, const float* raw1,
                                  const float* act1, const float* params_c, const float* packed_bwd_c, const float* params_f,
                                  const float* packed_bwd_f, float* draw_ws, float* dact_ws, float* partial_ws, float* grads_c,
                                  float* grads_f, const float* acc0, const float* depth0, const float* acc1, const float* depth1,
                                  const fn_map_grads* maps, fn_stream_t stream);
int fastnerf_render_rays_bwd_live_maps(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11,
                                       int white_bkgd, const float* g_rgb, const float* g_rgb0, const float* noise0,
                                       const float* noise1, const float* z0, const float* raw0, const float* z1,
                                       const float* raw1, const float* params_c, const float* packed_fwd_c,
                                       const float* packed_bwd_c, const float* params_f, const float* packed_fwd_f,
                                       const float* packed_bwd_f, float* draw_ws, float* act_ws, float* dact_ws,
                                       float* partial_ws, int32_t* live_ws, float* grads_c, float* grads_f, int32_t* counts_out,
                                       const float* acc0, const float* depth0, const float* acc1, const float* depth1,
                                       const fn_map_grads* maps, fn_stream_t stream);

/* ---- "bf16x6" math mode: fp32-WIDTH products on the bf16 matrix cores (csrc/mlp_*.hip, MM_X6) -------------------------------
 * Same network functions and call protocol as fastnerf_mlp_pack_ex / fwd_ex / fwd_flags_ex / bwd_ex / fwd_live_ex / bwd_live_ex
 * (run_nerf.py:50-64 run_network -> model.py:37-63, autograd backward of the same).  Every fp32 operand is decomposed EXACTLY
 * into three bf16 pieces (8 + 8 + 8 significand bits) and a product is the sum of the six piece products whose weight is
 * >= 2^-16 of it, accumulated in fp32 on the bf16 matrix cores (v_mfma_f32_16x16x32_bf16 in the forward / dX, v_mfma_f32_32x32x16_bf16 in dW): the dropped terms are <= 2^-24 of the product, the rounding
 * fp32 itself applies to it.  Weights are packed as three bf16 planes in the MFMA's fragment order (opaque; fastnerf_mlp_x6_packed_floats(kind, 1 | 2) floats);
 * saved activations / gradient workspaces are those of the exact-fp32 kernels (fastnerf_mlp_act_floats,
 * n*S*FASTNERF_DACT_FLOATS, fastnerf_mlp_bwd_partial_floats).  fwd: act == NULL -> inference, flags as
 * fastnerf_mlp_fwd_flags_ex (ignored when act != NULL). */
int64_t fastnerf_mlp_x6_packed_floats(int kind, int which);
int fastnerf_mlp_x6_pack(int kind, const float* params, float* packed_fwd, float* packed_bwd, fn_stream_t stream);
/* The fp32 / bf16x6 kernels run the feature (remap) layer and the view layer as ONE linear map of h7: M = Wv[:, :256] Wf, b' = bv + Wv[:, :256] bf,
 * folded in fp64 at every pack call.  The folded layer is appended to the packed buffers themselves, M^T to packed_bwd and the forward's part
 * to packed_fwd: a packed buffer is plain data, a pack call allocates nothing, and a copy of a packed buffer is as good as the original.  The
 * backward writes the gradients of both layers as before (an fp64 unfold behind the reduction).
 * fastnerf_mlp_fold_offset(kind, what): what = 0 [M | Wv[:, 256:]] in the view layer's forward order, 1 b' (128 plain floats), 2 M row-major
 * fp32 [128][256] -- offsets into packed_fwd, in floats of the fp32 packing (x 3/2 under bf16x6) --, 3 the offset of M^T in packed_bwd (same
 * units); anything else: -1. */
int64_t fastnerf_mlp_fold_offset(int kind, int what);
int fastnerf_mlp_x6_fwd(int kind, int64_t n, int S, const float* rays11, const float* z, const float* params,
                        const float* packed_fwd, float* raw, float* act, int flags, fn_stream_t stream);
int fastnerf_mlp_x6_bwd(int kind, int64_t n, int S, const float* draw, const float* act, const float* params,
                        const float* packed_bwd, float* dact, float* partial, float* grads, fn_stream_t stream);
int fastnerf_mlp_x6_fwd_live(int kind, int64_t n, int S, const float* rays11, const float* z, const float* params,
                             const float* packed_fwd, float* act, const int32_t* live_idx, const int32_t* live_cnt,
                             fn_stream_t stream);
int fastnerf_mlp_x6_bwd_live(int kind, int64_t n, int S, const float* draw, const float* act, const float* params,
                             const float* packed_bwd, float* dact, float* partial, float* grads, const int32_t* live_idx,
                             const int32_t* live_cnt, fn_stream_t stream);

/* ---- one optimisation step per call (run_nerf.py:479-508: render -> img2mse fine + coarse -> loss.backward() ->
 * optimizer.step(), the epoch loss map of :505-506 fed inside the loss launch) ----------------------------------------
 * fastnerf_train_step enqueues the phases selected by `phases` on `stream`, using exactly the entry points above in the
 * order the reference's loop implies, so its results are bit-identical to calling them one by one; what it removes is
 * host work (one call instead of ~10 and no per-step allocations: the caller keeps every buffer alive in `args`).
 * Data parallel: FN_STEP_FORWARD | FN_STEP_BWD_FINE, then the caller starts the all-reduce of the fine net's gradient
 * (grads + net_floats) on a side stream, FN_STEP_BWD_COARSE runs beside it, all-reduce of the coarse half, FN_STEP_UPDATE.
 * Two distinct NeRF nets with view directions (or one net when N_importance == 0); coarse net first in params / grads /
 * adam_m / adam_v (the order of `grad_vars`, run_nerf.py:87-97).  Buffer shapes are those of the individual entry points;
 * act0 / act1 are used by the plain backward (live == 0), act_ws / live_ws / counts by the compacted one (live != 0).
 * With `occ` set (a compacted step only: -1 with live == 0, whose backward has no list, and with sigma noise, which is added
 * before the relu so that a zero sigma is not a dead sample) a sample in a cell whose bit is clear gets raw = (0,0,0,0) without
 * the network being run; d(loss)/d(raw) of such a sample is exactly zero, so the live list is a subset of the occupied list. */
#define FN_STEP_FORWARD 1     /* pack rays, forward, loss + d(loss)/d(rgb maps) + leaf table */
#define FN_STEP_BWD_FINE 2    /* backward of the fine pass -> grads + net_floats (no-op when N_importance == 0) */
#define FN_STEP_BWD_COARSE 4  /* backward of the coarse pass -> grads */
#define FN_STEP_UPDATE 8      /* Adam over both nets + re-pack of their weights */
/* A bit of fn_step_args.fwd_flags, not an FN_FWD_* option: between fastnerf_pack_rays and the forward of FN_STEP_FORWARD, near and
 * far of every row of rays11 are clamped by fastnerf_occ_ray_bounds(occ, ..., write_back = 1) -- the bits as they are at this step,
 * nothing cached -- so the coarse depths spread over the occupied part of the ray.  Needs occ != NULL (-1 otherwise).  The step
 * masks the bit off before the flags go on to the forward; the backward phases read the clamped rays11 that the forward left. */
#define FN_STEP_TIGHTEN 2
struct fn_occ_grid; /* the occupancy grid, declared below */
typedef struct fn_step_args {
  /* the batch */
  int64_t n;
  const float *rays_o, *rays_d, *target;            /* [n,3] each */
  const float *t_rand, *u, *noise0, *noise1;        /* injected randoms or NULL (fastnerf_render_rays_fwd) */
  uint64_t seed0, seed1;
  const int32_t* leaf_tag;                          /* [n,2] or NULL */
  uint32_t* table;                                  /* leaf-error table or NULL */
  /* networks, optimiser state */
  int64_t net_floats;                               /* FASTNERF_NET_PARAMS */
  float *params, *grads, *adam_m, *adam_v;          /* (1 or 2) x net_floats */
  float *packed_fwd_c, *packed_bwd_c, *packed_fwd_f, *packed_bwd_f;
  /* tensors of the step (outputs of the forward, kept for the backward) */
  float *rays11, *z0, *raw0, *act0, *rgb0, *disp0, *acc0, *w0, *depth0;
  float *z1, *z_samples, *z_std, *raw1, *act1, *rgb1, *disp1, *acc1, *w1, *depth1;
  float *g_rgb, *g_rgb0, *loss2;                    /* [n,3], [n,3], [2] */
  float *draw_ws, *act_ws, *dact_ws, *partial_ws;   /* scratch, sized as for fastnerf_render_rays_bwd(_live) */
  int32_t *live_ws, *counts;                        /* compacted backward: scratch, optional int32[4] live / total counts */
  double focal, lr, beta1, beta2, eps;
  float near_plane, far_plane, grad_scale;
  int32_t math_mode;                                /* 0 exact fp32 MFMA, 1 split-bf16 (x3), 2 bf16x6 (fp32 width) */
  int32_t N_samples, N_importance, lindisp, perturb, white_bkgd, ndc, H, W;
  int32_t live;                                     /* != 0: forward without saving + compacted backward */
  int32_t fwd_flags;                                /* FN_FWD_* of the first forward of a compacted step | FN_STEP_TIGHTEN */
  int32_t max_leaves, adam_t;
  /* training through an occupancy grid (declared below; live != 0 and no sigma noise): the first forward of each pass runs over
   * the occupied samples only, as fastnerf_render_rays_fwd_occ does; occ_counts: NULL or 4 int32 = (occupied, total) of the
   * coarse pass, then of the fine pass.  NULL / NULL: the step without a grid. */
  const struct fn_occ_grid* occ;
  int32_t* occ_counts;
} fn_step_args;
int64_t fastnerf_step_args_size(void);              /* sizeof(fn_step_args): binding sanity check */
int fastnerf_train_step(const fn_step_args* args, int phases, fn_stream_t stream);
/* The step with depth / opacity supervision (fastnerf_aux_loss): total loss = mse(fine) + mse(coarse) + lambda_depth (Ld_1 + Ld_0)
 * + lambda_acc (La_1 + La_0), where the reference would add such terms to `loss` before loss.backward() (run_nerf.py:479-494).
 * fn_step_args keeps its size; what the terms need travels in fn_step_aux, given in EVERY phase call (the data-parallel step
 * splits the phases): FN_STEP_FORWARD runs fastnerf_aux_loss behind fastnerf_mse_leafmax with args->grad_scale, the backward
 * phases hand the gradient buffers of the terms whose target is set to the compositing backward (fn_map_grads).  Targets and
 * weights: [n] or NULL as in fastnerf_aux_loss; g_*: [n] each (the *0 ones unused with one pass); loss4: [4].
 * aux == NULL (or both targets NULL) is fastnerf_train_step launch for launch. */
typedef struct fn_step_aux {
  const float *depth_target, *depth_weight, *acc_target, *acc_weight;
  float *g_depth1, *g_acc1, *g_depth0, *g_acc0, *loss4;
  float lambda_depth, lambda_acc;
} fn_step_aux;
int64_t fastnerf_step_aux_size(void);               /* sizeof(fn_step_aux): binding sanity check */
int fastnerf_train_step_aux(const fn_step_args* args, const fn_step_aux* aux, int phases, fn_stream_t stream);

/* ---- exchange steps of the data-parallel path ---------------------------------------------------
 * One process per GPU; every rank renders its shard of the ray batch end to end.  The reference's strategies for contrast:
 * nn.DataParallel around the MLP (nerf-ours/run_nerf.py:70,82,90), torch DDP (nerf++-ours/ddp_train_nerf.py:150-184).
 * A PyTorch host gets the same collectives from torch.distributed (backend "nccl" = RCCL; parallel.py, the default route);
 * these entry points serve a host without it.  librccl is resolved at the first call, the library does not link against it.
 *   fastnerf_comm_unique_id   rank 0: a fresh RCCL id (FASTNERF_COMM_ID_BYTES bytes) to hand to every rank out of band
 *   fastnerf_comm_init        collective over all ranks, on the caller's current HIP device
 *   fastnerf_allreduce_grads  in place SUM over ranks of the flat fp32 gradient buffer (or a slice of it: the fine net's half
 *                             can go while the coarse net's backward runs on another stream), then * scale (1 / world for the
 *                             global-batch mean of img2mse, run_nerf_helpers.py:9); enqueued on `stream`, no host sync
 *   fastnerf_allreduce_leaf_table  in place MAX over ranks of the per-(image, leaf) table of fastnerf_mse_leafmax (uint32 bit
 *                             patterns of non-negative floats: exact, order independent => identical on 1 or 8 GPUs)
 *   fastnerf_allreduce_leaf_sumcount  in place SUM over ranks of the fp64 sums / int32 counts of fastnerf_leaf_sumcount (the
 *                             nerf++ fork's MEAN rule, nerf++-ours/tree.py:609-632); the sums hold multiples of 2^-30, so the
 *                             result is exact: bit-identical to one rank accumulating every ray
 *   fastnerf_leaf_table_reset / _read   zero the device table / copy it to the host as floats and wait for it (the split
 *                             rule of tree.py:629-652 runs on the host: fastnerf_tree_adjust)                              */
#define FASTNERF_COMM_ID_BYTES 128
typedef struct fn_comm fn_comm; /* opaque: one RCCL communicator */
int fastnerf_comm_unique_id(char* id);
int fastnerf_comm_init(fn_comm** out, const char* id, int rank, int world);
int fastnerf_comm_destroy(fn_comm* comm);
int fastnerf_allreduce_grads(fn_comm* comm, float* grads, int64_t n, float scale, fn_stream_t stream);
int fastnerf_allreduce_leaf_table(fn_comm* comm, uint32_t* table, int64_t n, fn_stream_t stream);
int fastnerf_allreduce_leaf_sumcount(fn_comm* comm, double* sum, int32_t* count, int64_t n, fn_stream_t stream);
int fastnerf_leaf_table_reset(uint32_t* table, int64_t n, fn_stream_t stream);
int fastnerf_leaf_table_read(const uint32_t* table, float* host_out, int64_t n, fn_stream_t stream);

/* ---- mesh extraction (extract_mesh.py:38-74: dense density query + mcubes.marching_cubes) ------------------------------
 * fastnerf_grid_points: rows p0 .. p0+n-1 of the point grid (xs[i], ys[j], zs[k]), p = (i*ny + j)*nz + k (torch.meshgrid
 * 'ij' order), written as rays11 [n,11] with o = the point and everything else 0 -- what run_network builds for explicit
 * points, so fastnerf_mlp_*_fwd with z = 0 evaluates the network there.  fastnerf_grid_sigma: out[q] = relu(raw[q*4+3]).
 * Marching cubes over vol [nx,ny,nz] float32 (C order, every dimension >= 2, finite values), inside = value > thr:
 *   vertices  one per grid edge whose endpoints lie on different sides, ordered by the lower endpoint's linear index, then
 *             axis i, j, k; position in index coordinates = lower endpoint + t along the edge's axis,
 *             t = (thr - v_a) / (v_b - v_a) in fp32 (the other two coordinates are exact integers).  float verts [V,3].
 *   triangles int32 tris [T,3] of vertex indices, ordered by cell ((nx-1)(ny-1)(nz-1) cells, C order), then table order;
 *             (v1-v0) x (v2-v0) points from inside to outside.  The table (fastnerf_mc_tables) closes every mesh: ambiguous
 *             faces separate the inside corners.
 * Protocol: ws = fastnerf_mc_ws_bytes(nx, ny, nz) bytes of device memory; fastnerf_mc_count writes counts_host[0] = V,
 * counts_host[1] = T and, an exception to the convention above, SYNCHRONISES (it waits for `stream`); it returns -1 when V or T
 * exceeds 2^31-1.  fastnerf_mc_emit, with the same vol / thr / ws and nothing in between, fills verts and tris.  No
 * atomics: the output is bit-identical from run to run.
 * fastnerf_mc_tables: tri_host [256*FASTNERF_MC_TRI_STRIDE] int8 (edge triples, -1 terminated), edge_host [256] uint16
 * (crossing-edge mask per case); host only. */
#define FASTNERF_MC_TRI_STRIDE 16
int fastnerf_grid_points(int64_t p0, int64_t n, const float* xs, int64_t nx, const float* ys, int64_t ny, const float* zs,
                         int64_t nz, float* rays11, fn_stream_t stream);
int fastnerf_grid_sigma(int64_t n, const float* raw, float* out, fn_stream_t stream);
int64_t fastnerf_mc_ws_bytes(int64_t nx, int64_t ny, int64_t nz);
int fastnerf_mc_count(const float* vol, int64_t nx, int64_t ny, int64_t nz, float thr, void* ws, int64_t* counts_host,
                      fn_stream_t stream);
int fastnerf_mc_emit(const float* vol, int64_t nx, int64_t ny, int64_t nz, float thr, void* ws, float* verts, int32_t* tris,
                     fn_stream_t stream);
int fastnerf_mc_tables(int8_t* tri_host, uint16_t* edge_host);


/* ---- occupancy grid: rendering (and, opted into, training) that does not evaluate the network in empty space -----------------------
 * The grid: a box [lo, hi) in the network's input space (world space, or NDC space for LLFF scenes) cut into
 * n[0] x n[1] x n[2] cells, one bit per cell (fastnerf_occ_words() uint32 words; the bit layout is the library's), and
 * `outside_occupied`.  The cell index of a point x along an axis is floor((x - lo) * inv), subtraction and product each
 * rounded to fp32, inv = n / (hi - lo) rounded to fp32 once by the caller.  A point whose index lies outside 0 .. n-1 on any
 * axis, a non-finite point included, takes `outside_occupied`.  The struct lives on the HOST; `words` is a device pointer.
 *   fastnerf_occ_build      vol: point volume [nx+1, ny+1, nz+1] float32 (what the dense density query of extract_mesh.py:38-61
 *                           gives).  A cell is occupied when one of its 8 corners is > threshold (the corners' maximum, for a
 *                           volume without NaNs); then every cell within `dilate` cells (Chebyshev distance, clipped at the box)
 *                           of an occupied one becomes occupied.  ws: 2 * fastnerf_occ_words() uint32 of scratch (NULL allowed
 *                           when dilate == 0).
 *   fastnerf_occ_from_mask  mask: [nx, ny, nz] bytes (C order), non-zero = occupied
 *   fastnerf_occ_query      pts [n,3] -> out [n] bytes, 1 = occupied
 *   fastnerf_occ_classify   the n * S samples x = o + d * z of a pass (rays11 [n,11], z [n,S]; one rounded multiply, one rounded
 *                           add, as the MLP kernels compute the point): live_idx[0 .. count) = ascending indices n_ray * S + s of
 *                           the occupied samples, count_out[0] = count, count_out[1] = n * S (device values, no host round
 *                           trip), and raw[p*4 .. p*4+3] = 0 for every other sample (raw may be NULL).  ws:
 *                           fastnerf_compact_ws_ints(n * S) int32.  The three launches of fastnerf_compact_live with another
 *                           predicate: deterministic, no atomics. */
typedef struct fn_occ_grid {
  const uint32_t* words; /* device */
  float lo[3], inv[3];
  int32_t n[3];
  int32_t outside_occupied;
} fn_occ_grid;
int64_t fastnerf_occ_words(int64_t nx, int64_t ny, int64_t nz);
int fastnerf_occ_build(const float* vol, int64_t nx, int64_t ny, int64_t nz, float threshold, int dilate, uint32_t* words,
                       uint32_t* ws, fn_stream_t stream);
int fastnerf_occ_from_mask(const uint8_t* mask, int64_t nx, int64_t ny, int64_t nz, uint32_t* words, fn_stream_t stream);
int fastnerf_occ_query(const fn_occ_grid* grid, int64_t n, const float* pts, uint8_t* out, fn_stream_t stream);
int fastnerf_occ_classify(const fn_occ_grid* grid, int64_t n, int S, const float* rays11, const float* z, int32_t* live_idx,
                          int32_t* count_out, float* raw, int32_t* ws, fn_stream_t stream);
/* ---- cascade: an ordered list of 1 to 8 such grids g_0 .. g_{L-1} (usually the fine grid over the object, then coarser grids over
 * boxes around it; the boxes need not be nested or concentric), each with its own box, cell counts and bits.  A point is looked up
 * level by level, with each level's own index arithmetic as above: the FIRST level whose index lies in 0 .. n-1 on all three axes
 * decides, and the sample takes that cell's bit.  A point no level contains -- every non-finite point -- takes `outside_occupied` of
 * the LAST level; the `outside_occupied` of the other levels is not read.  A cascade of one level is that grid, bit for bit.  The
 * struct lives on the HOST; level[l].words are device pointers.  fn_occ_grid and fn_step_args keep their sizes: the cascade has
 * entry points of its own.  Training takes a cascade too, as one more trailing pointer of the step (fastnerf_train_step_cascade /
 * fastnerf_train_step_march_cascade below; fn_step_args.occ stays a single grid and is NULL then), refreshed over the own cells of
 * its levels ("cascade, trained" below).
 *   fastnerf_occ_query_cascade     the arguments and the result of fastnerf_occ_query
 *   fastnerf_occ_classify_cascade  the contract of fastnerf_occ_classify: ascending list, device count, zero logits for the other
 *                                  samples, the same ws, the same three launches without atomics
 * -1 unless 1 <= levels <= FN_OCC_MAX_LEVELS and every level passes the checks fastnerf_occ_query makes of its grid. */
#define FN_OCC_MAX_LEVELS 8
typedef struct fn_occ_cascade {
  int32_t levels;
  int32_t reserved;
  fn_occ_grid level[FN_OCC_MAX_LEVELS];
} fn_occ_cascade;
int fastnerf_occ_query_cascade(const fn_occ_cascade* cascade, int64_t n, const float* pts, uint8_t* out, fn_stream_t stream);
int fastnerf_occ_classify_cascade(const fn_occ_cascade* cascade, int64_t n, int S, const float* rays11, const float* z,
                                  int32_t* live_idx, int32_t* count_out, float* raw, int32_t* ws, fn_stream_t stream);
/* A grid that is kept while the networks train (fn_step_args.occ): a persistent density dens[nx*ny*nz] (fp32, cell order
 * c = (i*ny + j)*nz + k) beside the bits.
 *   fastnerf_occ_cell_points  one point inside each of the cells c0 .. c0+n-1, as rays11 rows [n,11] in the layout of
 *                           fastnerf_grid_points (o = point, everything else 0).  Per axis x = lo + (index + jitter) / inv, each
 *                           operation rounded to fp32; jitter = 0.5 when seed == 0, else a Philox4x32-10 draw in [0,1) keyed by
 *                           (seed, cell): the same seed gives the same bits.  Where rounding would put x into a neighbouring cell
 *                           the jitter is clamped towards 0.5, so that fastnerf_occ_query of the point names the cell (for every
 *                           grid whose cells are wider than a few fp32 steps of their coordinates).  grid->words is not read.
 *   fastnerf_occ_update     raw_c / raw_f: [n,4] logits of the coarse / fine network (raw_f may be NULL) at the points of the
 *                           cells c0 .. c0+n-1.  dens[c] = max(dens[c] * decay, relu(sigma_c), relu(sigma_f)) for those cells
 *                           (a NaN sigma counts as 0), every other cell keeps its value; then, in the same launch, the bit of
 *                           EVERY cell becomes dens > threshold, and the dilation of fastnerf_occ_build follows.  ws: 2 *
 *                           fastnerf_occ_words() uint32 (NULL allowed when dilate == 0).  n == 0 re-derives the bits only;
 *                           words == NULL updates the density only (a refresh in several chunks derives the bits once, at its
 *                           end). */
int fastnerf_occ_cell_points(const fn_occ_grid* grid, int64_t c0, int64_t n, uint64_t seed, float* rays11, fn_stream_t stream);
int fastnerf_occ_update(const float* raw_c, const float* raw_f, int64_t c0, int64_t n, int64_t nx, int64_t ny, int64_t nz,
                        float decay, float threshold, int dilate, float* dens, uint32_t* words, uint32_t* ws, fn_stream_t stream);
/* ---- cascade, trained: a cascade whose levels each carry a density, refreshed over the cells a lookup can read.  A lookup gives a
 * point to the FIRST level whose box contains it, so a cell of level l well inside the box of a level j < l is never read.
 * Own cells.  In float64, from each level's fp32 lo, inv and n: w = 1 / (double)inv, hi = lo + n w, every product and sum rounded on
 * its own.  Cell (i0, i1, i2) of level l is COVERED when there is ONE level j < l with, on every axis a and m = dilate + 1,
 *   lo_l[a] + (i_a - m) w_l[a] >= lo_j[a] + w_j[a]     and     lo_l[a] + (i_a + 1 + m) w_l[a] <= hi_j[a] - w_j[a];
 * every other cell is an OWN cell of l.  Level 0 owns all its cells; a cell covered only by a union of inner boxes is own
 * (conservative; the boxes need not be nested).  With n[a] <= 4096 the fp32 index of a point is within 0.001 cell of the real one,
 * so a point whose cell at level l is covered lies 0.99 w_j inside box j and is decided by a level <= j: a covered cell is never
 * read, and the margin m keeps every cell within `dilate` of a readable one sampled.
 *   fastnerf_occ_cascade_own     list[0 .. count) = the ascending cell indices of `level`'s own cells, count_out = (count, cells
 *                                of the level) on the device.  list: room for every cell of the level; ws:
 *                                fastnerf_compact_ws_ints(cells).  The covered intervals are worked out on the host; the device
 *                                runs the count / scan / scatter of fastnerf_occ_classify with that predicate: no atomics, the
 *                                same bits from call to call.  words are not read.
 * The refresh runs over the CONCATENATION of the levels' own lists, level 0 first: own[offsets[l] .. offsets[l+1]) is level l's list,
 * offsets[levels + 1] on the host.
 *   fastnerf_occ_cascade_points  one rays11 row per position q0 .. q0+n-1: the point fastnerf_occ_cell_points makes for that
 *                                level's grid and that cell, bit for bit (same Philox key (seed, cell), same clamping, seed == 0
 *                                gives centres).  One launch serves a range that spans levels.
 *   fastnerf_occ_cascade_update  dens_l[cell] = max(dens_l[cell] * decay[l], relu(sigma_c), relu(sigma_f)) for the positions q0 ..
 *                                q0+n-1 (raw_c / raw_f [n,4] as for fastnerf_occ_update; a NaN counts as 0).  decay[levels] and
 *                                dens[levels] (device pointers) are HOST arrays.  A cell stands once in the concatenation: plain
 *                                stores, no atomics.  The bits and their dilation follow per level from fastnerf_occ_update(n = 0);
 *                                a covered cell keeps dens = 0, so its bit is clear.
 * -1 before anything is enqueued: levels outside 1 .. 8, a level with n[a] outside 1 .. 4096, a non-finite lo or inv <= 0; level or
 * dilate out of range; offsets that do not start at 0, descend, or give a level more entries than it has cells; a range outside the
 * concatenation; a NULL pointer that would be read. */
int fastnerf_occ_cascade_own(const fn_occ_cascade* cascade, int level, int dilate, int32_t* list, int32_t* count_out, int32_t* ws,
                             fn_stream_t stream);
int fastnerf_occ_cascade_points(const fn_occ_cascade* cascade, const int32_t* own, const int64_t* offsets, int64_t q0, int64_t n,
                                uint64_t seed, float* rays11, fn_stream_t stream);
int fastnerf_occ_cascade_update(const fn_occ_cascade* cascade, const float* raw_c, const float* raw_f, const int32_t* own,
                                const int64_t* offsets, int64_t q0, int64_t n, const float* decay, float* const* dens,
                                fn_stream_t stream);
/* NeRF.forward + Embedder.embed (model.py:38-63) of the points live_idx[0 .. *live_cnt) only, inference (nothing saved):
 * raw[live_idx[j]*4 .. +3] = the logits the plain forward gives that point; no other element of raw is written.  kind 0 only.
 * flags as fastnerf_mlp_fwd_flags_ex, a tile being 64 consecutive list entries.  _ex: exact fp32, bf16: split-bf16 (x3),
 * x6: bf16x6. */
int fastnerf_mlp_fwd_list_ex(int kind, int64_t n, int S, const float* rays11, const float* z, const float* params,
                             const float* packed_fwd, float* raw, const int32_t* live_idx, const int32_t* live_cnt, int flags,
                             fn_stream_t stream);
int fastnerf_mlp_bf16_fwd_list(int kind, int64_t n, int S, const float* rays11, const float* z, const float* params,
                               const float* packed_fwd, float* raw, const int32_t* live_idx, const int32_t* live_cnt, int flags,
                               fn_stream_t stream);
int fastnerf_mlp_x6_fwd_list(int kind, int64_t n, int S, const float* rays11, const float* z, const float* params,
                             const float* packed_fwd, float* raw, const int32_t* live_idx, const int32_t* live_cnt, int flags,
                             fn_stream_t stream);
/* render_rays (render.py:195-305) through an occupancy grid, inference only: what fastnerf_render_rays_fwd_ex enqueues with
 * act0 == act1 == NULL and no sigma noise, except that each MLP launch becomes fastnerf_occ_classify + the list forward: a
 * sample in a cell whose bit is clear gets raw = (0, 0, 0, 0) without the network being evaluated, in both passes (the coarse
 * weights that feed the inverse-CDF sampler come from the masked logits).  An occupied sample gets exactly the logits of the
 * plain forward.  live_ws: n * (N_samples + N_importance) + fastnerf_compact_ws_ints(n * (N_samples + N_importance)) int32 of
 * scratch; counts_out: 4 int32 = (occupied, total) of the coarse pass, then of the fine pass. */
int fastnerf_render_rays_fwd_occ(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11, int lindisp,
                                 int perturb, int det, int white_bkgd, const float* t_rand, const float* u, uint64_t seed0,
                                 uint64_t seed1, const float* params_c, const float* packed_c, const float* params_f,
                                 const float* packed_f, const fn_occ_grid* grid, int32_t* live_ws, int32_t* counts_out, float* z0,
                                 float* raw0, float* rgb0, float* disp0, float* acc0, float* w0, float* depth0, float* z1,
                                 float* z_samples, float* z_std, float* raw1, float* rgb1, float* disp1, float* acc1, float* w1,
                                 float* depth1, int flags, fn_stream_t stream);
/* The same through a cascade: every argument as above, each pass sorted by fastnerf_occ_classify_cascade.  The two functions share
 * one body; with levels == 1 the outputs equal fastnerf_render_rays_fwd_occ's with that grid bit for bit. */
int fastnerf_render_rays_fwd_occ_cascade(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11, int lindisp,
                                         int perturb, int det, int white_bkgd, const float* t_rand, const float* u, uint64_t seed0,
                                         uint64_t seed1, const float* params_c, const float* packed_c, const float* params_f,
                                         const float* packed_f, const fn_occ_cascade* cascade, int32_t* live_ws, int32_t* counts_out,
                                         float* z0, float* raw0, float* rgb0, float* disp0, float* acc0, float* w0, float* depth0,
                                         float* z1, float* z_samples, float* z_std, float* raw1, float* rgb1, float* disp1,
                                         float* acc1, float* w1, float* depth1, int flags, fn_stream_t stream);

/* ---- early ray termination (inference): stop evaluating the network on a ray once it is opaque ---------------------------------------
 * `ert = eps`, 0 <= eps < 1, with `ert_block = B` >= 1.  The image pass is the fine pass when N_importance > 0 and the only pass
 * otherwise.  Its S sorted samples of every ray are cut into segments of B consecutive sample indices [kB, min((k+1)B, S)).  Per
 * ray a transmittance T is kept in fp32, starting at 1; after segment k has its logits, T is multiplied by the segment's product of
 * (1 - alpha_i + 1e-10), alpha_i = 1 - exp(-relu(sigma_i) dist_i), dist_i = z_{i+1} - z_i (1e10 for the ray's last sample) times
 * |d|, each formed with the rounded operations of fastnerf_raw2outputs_fwd.  A sample of segment k is evaluated when its ray's T at
 * the START of the segment is > eps and, if a grid or a cascade is given, its occupancy bit is set; every other sample of the segment
 * gets raw = (0, 0, 0, 0) without the network.  An evaluated sample gets exactly the logits of the plain forward (rows of the matrix
 * products do not see each other).  Compositing is the unchanged fastnerf_raw2outputs_fwd over the whole raw.
 * The coarse pass of a two-pass render is not touched: it runs plain, or through the grid / cascade, as without `ert`, so z0, raw0,
 * the coarse maps, z1, z_samples and z_std are bit-identical to the same call without `ert`.
 * Consequences: the skipped samples of a ray carry a total weight <= T_start (1 + S 1e-10) <= eps in the plain render, hence
 * |d rgb_map| <= eps per channel (with or without white_bkgd), 0 <= acc_plain - acc_ert <= eps, |d depth_map| <= eps z_max; disp_map
 * (a quotient) has no such bound.  With eps = 0 a segment is skipped only once T has underflowed to exactly 0 and every map equals
 * the plain call's bit for bit; with B >= S there is one segment, nothing is skipped, and every output, raw included, equals that of
 * fastnerf_render_rays_fwd_occ / _occ_cascade (a grid / cascade) or of the plain non-saving forward (neither).
 *   fastnerf_ert_classify  one segment [s0, s1) of a pass of n * S samples: live_idx[0 .. count) = ascending indices ray * S + s,
 *                          s0 <= s < s1, of the samples whose ray has trans[ray] > eps (trans == NULL: every ray; a NaN is not >
 *                          eps) and whose bit is set in `grid` / `cascade` (at most one non-NULL; neither: every sample);
 *                          count_out[0] = count, count_out[1] = n * (s1 - s0); raw[p*4 .. p*4+3] = 0 for the segment's other
 *                          samples (raw may be NULL), nothing outside the segment is written.  ws: fastnerf_compact_ws_ints(n *
 *                          (s1 - s0)) int32.  The three launches of fastnerf_occ_classify with another descriptor: no atomics.
 *   fastnerf_ert_advance   trans[ray] = (first ? 1 : trans[ray]) * prod over s0 <= s < s1 of (1 - alpha_s + 1e-10) from raw, z and
 *                          rays11 as above (S <= 512); total (may be NULL): total[0] = (first ? 0 : total[0]) + seg_count[0],
 *                          total[1] = n * S.  One launch, one wave per ray, plain stores.
 *   fastnerf_render_rays_fwd_ert  the arguments of fastnerf_render_rays_fwd_occ with `grid` AND `cascade` (at most one non-NULL, both
 *                          may be NULL), eps, block = B and trans_ws (n floats: on return the image pass's final T per ray).  The
 *                          coarse pass of two: as fastnerf_render_rays_fwd_occ / _occ_cascade, or the plain forward with neither.
 *                          The image pass: per segment fastnerf_ert_classify + the list forward + fastnerf_ert_advance (4 launches
 *                          beside the list forward).  live_ws: the int32 of fastnerf_render_rays_fwd_occ + 2.  counts_out: 4 int32 =
 *                          (evaluated, total) of the coarse pass, then of the fine pass (one pass: the first pair only).  A
 *                          coarse pass that runs plain (neither grid nor cascade) evaluates every sample and writes NOTHING
 *                          to its pair: (n * N_samples, n * N_samples) is known to the caller.
 *                          -1 before anything is enqueued unless 0 <= eps < 1, block >= 1, n * (N_samples + N_importance) < 2^31,
 *                          the pointers are set and the cascade passes its checks. */
int fastnerf_ert_classify(const fn_occ_grid* grid, const fn_occ_cascade* cascade, int64_t n, int S, int s0, int s1, const float* rays11,
                          const float* z, const float* trans, float eps, int32_t* live_idx, int32_t* count_out, float* raw,
                          int32_t* ws, fn_stream_t stream);
int fastnerf_ert_advance(int64_t n, int S, int s0, int s1, const float* raw, const float* z, const float* rays11, int first,
                         float* trans, const int32_t* seg_count, int32_t* total, fn_stream_t stream);
int fastnerf_render_rays_fwd_ert(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11, int lindisp,
                                 int perturb, int det, int white_bkgd, const float* t_rand, const float* u, uint64_t seed0,
                                 uint64_t seed1, const float* params_c, const float* packed_c, const float* params_f,
                                 const float* packed_f, const fn_occ_grid* grid, const fn_occ_cascade* cascade, float eps, int block,
                                 float* trans_ws, int32_t* live_ws, int32_t* counts_out, float* z0, float* raw0, float* rgb0,
                                 float* disp0, float* acc0, float* w0, float* depth0, float* z1, float* z_samples, float* z_std,
                                 float* raw1, float* rgb1, float* disp1, float* acc1, float* w1, float* depth1, int flags,
                                 fn_stream_t stream);

/* ---- per-ray bounds from the occupancy grid: do not PLACE samples in empty space (csrc/ray_bounds.hip) ---------------------------------
 * Row r of rays11 [n,11] gives o, d, near (column 6) and far (column 7) in the space the grid lives in (NDC space for NDC batches:
 * where the samples are looked up).  Per ray (near', far', hit) through `grid` or `cascade` (exactly one non-NULL):
 *   conservative  for every depth near <= z <= far whose sample x = o + d * z (one rounded multiply, one rounded add, as
 *                 fastnerf_occ_classify forms it) the lookup calls occupied: hit = 1 and near' <= z <= far'.  No exceptions:
 *                 `outside_occupied` is honoured, so stretches of [near, far] outside every box count as occupied when it is set --
 *                 such a grid tightens little; outside_occupied = 0 is the configuration this is for.
 *   tight         near <= near' < far' <= far, and near' / far' lie less than a cell (the width of the fp32 uncertainty of a face
 *                 crossing, see ray_bounds.hip) before the first / after the last cell of the ray that is occupied.
 *   unchanged     near' = near, far' = far when the ray meets no occupied stretch in [near, far] (hit = 0), and, with hit = 1, when
 *                 the clamped interval would be empty or a point, when o, d, near or far is not finite, when near >= far, when the
 *                 ray's terms are too large for the rounding bound (|o|, |d| far or the cell counts beyond some 2^18 cells), or when
 *                 the iteration cap -- 2 (nx + ny + nz) + 16 per level, + 16, computed by this call -- is reached.  Unchanged
 *                 bounds with hit = 1 are always a valid answer.
 * bounds [n,2] (near', far') and hit [n] bytes may each be NULL; write_back != 0 also stores near' / far' into columns 6 / 7 of
 * the row -- no other column is written, and a ray whose bounds are unchanged is not written at all.  One launch, one thread per
 * ray, no atomics, no scratch: the result is bit-identical from run to run, and a cascade of one level gives the grid's bits.
 * Not differentiable: near' and far' are constants of a backward, as near and far are. */
int fastnerf_occ_ray_bounds(const fn_occ_grid* grid, const fn_occ_cascade* cascade, int64_t n, float* rays11, int write_back,
                            float* bounds, uint8_t* hit, fn_stream_t stream);

/* ---- marched render (inference): walk a dense lattice of depths through the grid, evaluate ONE network on the occupied ones ------------
 * (csrc/march.hip; no sampler, no coarse pass, no inverse-CDF.)
 * Lattice.  A ray has K lattice depths, 2 <= K < 2^24: z_k = the depth fastnerf_sample_coarse gives sample k for S = K, perturb = 0 (the
 * same device function, hence the same bits), k = 0 .. K-1, and z_K := z_{K-1} + (z_{K-1} - z_{K-2}), each operation rounded to fp32:
 * the closing depth of the last lattice point.
 * Live.  live(k) is the lookup of fastnerf_occ_classify / _classify_cascade at x = o + d * z_k (one rounded multiply, one rounded add),
 * through `grid` or `cascade` (exactly one non-NULL) with their `outside_occupied`.  Nothing conservative: the live set is exactly the
 * live list that a dense classify of the K lattice depths produces.
 * Packed sequence.  For every maximal run a .. b of consecutive live lattice points the ray has the entries (z_a, a), ..., (z_b, b) and
 * one closing entry (z_{b+1}, -1); the runs follow each other in depth order.  The closing entry carries zero logits and is never
 * evaluated: it gives sample b the width z_{b+1} - z_b that it has in the dense pass instead of the gap to the next run.
 * Packed row.  C slots, 2 <= C <= 512: z [n,C] float32, kidx [n,C] int32, raw [n,C,4].  The first min(L, C) entries of the sequence (of
 * length L) are stored.  When L > C the last kept entry's kidx is -1 (its z stays) and overflow[ray] = 1, else 0: slot C-1 never holds a
 * live sample (fastnerf_raw2outputs_fwd gives a row's last slot the width 1e10).  The remaining slots are padding, (z of the slot
 * before, -1); a ray without a live lattice point holds (z_0, -1) throughout.  z is non-decreasing along a row wherever the lattice is.
 * Rounds.  The row is produced in rounds over consecutive segments [s0, s1) of its slots -- one round [0, C) without early ray termination,
 * segments of B slots with `ert = eps`, `ert_block = B`.  A ray whose transmittance (fastnerf_ert_advance over the packed row) at the
 * start of segment j is not > eps is cut at slot jB: if slot jB-1 holds live sample k, slot jB still receives its closing entry
 * (z_{k+1}, -1); everything after is padding, the ray's lattice position does not advance, and its overflow flag is what the earlier
 * rounds left.  Every round with s1 < C also stores z[s1]: z_{k+1} when slot s1-1 holds live sample k (that IS the depth of the next
 * entry, whatever it turns out to be), else the padding depth; fastnerf_ert_advance of the segment reads it for the width of slot s1-1,
 * and the next round overwrites it only with the depth of a new run after a gap, behind a slot whose logits are zero.  With B >= C the
 * arrays, maps and raw equal those without ert bit for bit; with eps = 0 every map does; otherwise the bounds of the early-ray-
 * termination block hold against the marched render without ert, by the same argument (|d rgb_map| <= eps, 0 <= d acc <= eps,
 * |d depth_map| <= eps z_max).
 * Consequence.  For a ray without overflow whose lattice point K-1 is not live, the packed row is the dense one-pass render through the
 * grid at N_samples = K (fastnerf_render_rays_fwd_occ, N_importance = 0, perturb = 0) with its empty samples dropped: the evaluated
 * logits are bit-identical, every live sample has the same width bits, and the maps differ only by the grouping of the fp32 scan and
 * sums.  A live K-1 is closed at z_K here and gets 1e10 there.
 *   fastnerf_occ_march   one round [s0, s1) for all rays, `first` exactly when s0 == 0.  state: 2 int32 per ray of caller scratch, written
 *                        by the first round and carried between rounds -- the next lattice index, and (bit 0) whether slot s1-1 is live,
 *                        (bits 1..5) the lookups made and not yet consumed: over all rounds a ray makes at most K lookups.  trans (may be
 *                        NULL: no ray is cut), eps as fastnerf_ert_classify.  Outputs z, kidx, overflow (n bytes).  One launch, one thread
 *                        per ray, no atomics: bit-identical from run to run.  At most s1 - s0 + 1 slots are written per ray, every index
 *                        < C, and the walk ends after at most K steps whatever the rays hold (non-finite, near >= far: such rays get the
 *                        rows that the lookup's answers imply).
 *   fastnerf_march_list  the live list of segment [s0, s1): live_idx[0 .. count) = ascending ray * C + slot with kidx >= 0, count_out[0]
 *                        = count, count_out[1] = n * (s1 - s0); raw[p*4 .. +3] = 0 for the segment's other slots (raw may be NULL).  ws:
 *                        fastnerf_compact_ws_ints(n * (s1 - s0)) int32.  The launches of fastnerf_occ_classify with another descriptor.
 *                        total (may be NULL): total[0] = (s0 == 0 ? 0 : total[0]) + count, total[1] = lattice.
 *   fastnerf_render_rays_fwd_march  per round march + list + fastnerf_mlp_*_fwd_list on the packed z with S = C (+ fastnerf_ert_advance
 *                        while a further round follows), then one fastnerf_raw2outputs_fwd over [n, C].  block = 0: no early ray
 *                        termination; else eps, block as fastnerf_render_rays_fwd_ert.  params / packed: the one network.  counts_out:
 *                        2 int32 = (evaluated samples, n * K).  The scratch is the stream's library-owned workspace.  -1 before
 *                        anything is enqueued unless math_mode in {0,1,2}, 2 <= K < 2^24, 2 <= C <= 512, n * C and n * K < 2^31, the
 *                        ert arguments are in range, exactly one of grid / cascade is set and passes its checks, the pointers are set,
 *                        and the workspace is there (not inside a stream capture). */
int fastnerf_occ_march(const fn_occ_grid* grid, const fn_occ_cascade* cascade, int64_t n, int K, int lindisp, const float* rays11, int C,
                       int s0, int s1, int first, const float* trans, float eps, int32_t* state, float* z, int32_t* kidx,
                       uint8_t* overflow, fn_stream_t stream);
int fastnerf_march_list(int64_t n, int C, int s0, int s1, const int32_t* kidx, int32_t* live_idx, int32_t* count_out, float* raw,
                        int32_t* ws, int32_t* total, int32_t lattice, fn_stream_t stream);
int fastnerf_render_rays_fwd_march(int math_mode, int64_t n, int K, int C, const float* rays11, int lindisp, int white_bkgd,
                                   const float* params, const float* packed, const fn_occ_grid* grid, const fn_occ_cascade* cascade,
                                   float eps, int block, int32_t* counts_out, float* z, int32_t* kidx, uint8_t* overflow, float* raw,
                                   float* rgb, float* disp, float* acc, float* w, float* depth, int flags, fn_stream_t stream);

/* ---- marched training: the lattice jittered per ray, ONE network trained on the packed rows ----------------------------------------
 * (csrc/march.hip, render.cpp.)  A lattice sampled at the same depths every step fits those depths only, so training shifts the whole
 * lattice of ray r by u_r in [0, 1) of its own spacing:
 *   z_k(u) = fadd(z_k, fmul(u_r, fsub(z_{k+1}, z_k)))     k = 0 .. K-1   (z_k, z_K: the lattice and closing depth of the marched render)
 *   z_K(u) = fadd(z_{K-1}(u), fsub(z_K, z_{K-1}))
 * for the linear and the lindisp lattice alike, each operation rounded to fp32.  The lookup is made at o + d * z_k(u), the stored depths
 * are the z_k(u), a closing entry after sample b stores z_{b+1}(u); runs, closing entries, padding, overflow, rounds and state are
 * exactly those of fastnerf_occ_march.  z_k <= z_k(u) <= z_{k+1} on the linear lattice, and z stays non-decreasing along a row.
 *   fastnerf_occ_march_jitter  the arguments of fastnerf_occ_march plus u ([n] or NULL) and seed.  u given: used as it is.  u == NULL,
 *                        seed != 0: u_r = u01(word 0) of Philox block r of the stream 'mrch' (0x6d726368) keyed by seed.  u == NULL, seed
 *                        == 0: no shift -- the launch of fastnerf_occ_march itself.  With u_r = 0 every z_k(u) has the bits of z_k (finite
 *                        rays with 0 < near < far: u_r * w = 0, and a + ((a + w) - a) = a + w since a <= a + w <= 2a makes the difference
 *                        exact), so z, kidx, overflow and state equal fastnerf_occ_march's bit for bit.  One thread per ray, no atomics:
 *                        bit-identical from run to run; the bounds of fastnerf_occ_march hold (the same walk).
 *   fastnerf_march_mask  g_rgb [n,3]: row r is zeroed where overflow[r] != 0, every other row keeps its bits.  A truncated row has lost
 *                        everything behind the cut: its colour error is an artefact of the row, not of the field.
 *   fastnerf_train_step_march  one optimisation step of the marched network per call, phases as fastnerf_train_step:
 *     FN_STEP_FORWARD     fastnerf_pack_rays, (FN_STEP_TIGHTEN: fastnerf_occ_ray_bounds, write_back = 1,) one round [0, C) of
 *                         fastnerf_occ_march_jitter, fastnerf_march_list, fastnerf_mlp_*_fwd_list of the mode with S = C,
 *                         fastnerf_raw2outputs_fwd over [n, C], fastnerf_mse_leafmax(rgb, NULL, target, ...), fastnerf_march_mask.
 *                         loss2[0] stays the mean over all n rays and grad_scale is unchanged.
 *     FN_STEP_BWD_COARSE  the compacted backward (fastnerf_render_rays_bwd_live) over the row as N_samples = C, N_importance = 0, into
 *                         the marched half of grads: a closing or padding slot has raw = (0,0,0,0), d(loss)/d(raw) is exactly zero
 *                         there, so its list is a subset of the row's live slots.  FN_STEP_BWD_FINE is a no-op.
 *     FN_STEP_UPDATE      fastnerf_adam_step over the marched half of params / grads / adam_m / adam_v and the pack of that network.
 *                         The other network, its moments and its packed buffers are not touched.
 *   Exactly the launches those entry points make, in that order, on the caller's stream: bit-identical to calling them one by one.
 *   No early ray termination (one round) and no depth / opacity terms.  fn_step_args keeps its size and meaning; of it the step reads
 *   the batch, the networks and optimiser state, rays11, the row buffers z0 raw0 rgb0 disp0 acc0 w0 depth0 sized for [n, C], g_rgb,
 *   loss2, the scratch of the compacted backward sized for n * C points, counts, the scalars and occ; N_samples, N_importance, t_rand,
 *   u, seed0 and seed1 are NOT read.  What the march needs travels in fn_step_march, given in every phase call.
 *   -1 before anything is enqueued: occ == NULL or a grid that fails its checks, live == 0, sigma noise, K / C outside the bounds of
 *   fastnerf_render_rays_fwd_march, which outside {0, 1}, a missing buffer of a requested phase. */
typedef struct fn_step_march {
  int32_t K, C;                 /* lattice depths per ray, slots per packed row */
  int32_t which;                /* 0 / 1: the half of params, grads, adam_m, adam_v and the packed pair (_c / _f) that is marched */
  const float* u;               /* [n] injected shifts or NULL */
  uint64_t seed;                /* u == NULL: the key of the 'mrch' stream, 0 = no shift */
  int32_t* kidx;                /* [n, C] out */
  uint8_t* overflow;            /* [n] out */
  int32_t* list_ws;             /* fastnerf_step_march_ws_ints(n, C) int32: list | scan scratch | count | per-ray state */
  int32_t* counts;              /* int32[2] out = (evaluated samples, n * K) */
} fn_step_march;
int64_t fastnerf_step_march_size(void);             /* sizeof(fn_step_march): binding sanity check */
int64_t fastnerf_step_march_ws_ints(int64_t n, int C);   /* -1 outside n > 0, 2 <= C <= 512, n * C < 2^31 */
int fastnerf_occ_march_jitter(const fn_occ_grid* grid, const fn_occ_cascade* cascade, int64_t n, int K, int lindisp, const float* rays11,
                              int C, int s0, int s1, int first, const float* trans, float eps, const float* u, uint64_t seed,
                              int32_t* state, float* z, int32_t* kidx, uint8_t* overflow, fn_stream_t stream);
int fastnerf_march_mask(int64_t n, const uint8_t* overflow, float* g_rgb, fn_stream_t stream);
int fastnerf_train_step_march(const fn_step_args* args, const fn_step_march* march, int phases, fn_stream_t stream);

/* ---- per-ray background colours (csrc/bkgd.hip, render.cpp) --------------------------------------------------------------------------
 * With ONE fixed background (white_bkgd) a pixel of that colour is explained as well by fog of that colour as by empty space.  Here
 * every ray r gets its own colour b_r behind both the prediction and an RGBA target, fresh every step: density where the image is
 * transparent then always costs.  The compositing runs with white_bkgd = 0 and knows nothing of it:
 *   fastnerf_bkgd_blend   b_r = bkgd[r], or with bkgd == NULL (u01(w0), u01(w1), u01(w2)) of Philox block r (counter (r lo, r hi, 'bkgd' =
 *                         0x626b6764, 0), key seed) -- exactly one of bkgd != NULL and seed != 0, -1 otherwise.  In place, for the image
 *                         pass (rgb1, acc1) and, when given, the coarse pass (rgb0, acc0):
 *                           rgb_k[r][c] = fadd(rgb_k[r][c], fmul(fsub(1, acc_k[r]), b_r[c]))
 *                           target_out[r][c] = alpha ? fadd(fmul(target[r][c], alpha[r]), fmul(fsub(1, alpha[r]), b_r[c])) : target[r][c]
 *                           bkgd_used[r] = b_r
 *                         With b = 1 the colour line has the bits of the white branch of fastnerf_raw2outputs_fwd.
 *   fastnerf_bkgd_grad    x = fadd(fadd(fmul(g0, b0), fmul(g1, b1)), fmul(g2, b2)) of g_rgb_k[r] and bkgd_used[r];
 *                         g_acc_k[r] = add_k ? fsub(add_k[r], x) : -x      (add_k: another term's d(loss)/d(acc), e.g. the opacity term's;
 *                         add_k == g_acc_k is allowed).  The row goes to fastnerf_raw2outputs_bwd_full beside g_rgb, white_bkgd = 0.
 * One thread per ray, no atomics: bit-identical from call to call.  n == 0 returns 0.
 *   fastnerf_train_step_bkgd / fastnerf_train_step_march_bkgd   fastnerf_train_step_aux / fastnerf_train_step_march with a background:
 *     FN_STEP_FORWARD  the forward as before, fastnerf_bkgd_blend(bkgd, seed, alpha, ...) on its colour maps and the target into target_ws,
 *                      fastnerf_mse_leafmax on the blended maps against target_ws (the leaf-error table sees what the loss sees),
 *                      fastnerf_aux_loss when a term is on, (marched: fastnerf_march_mask, and only then) fastnerf_bkgd_grad into g_acc1 /
 *                      g_acc0, with add_k = the opacity term's rows when that term is on.  An overflowed ray of a marched row so gets
 *                      g_acc = +-0.
 *     backward phases  g_acc1 / g_acc0 go to the full-gradient compositing backward of their pass beside the colour gradient.
 *   fn_step_bkgd is given in EVERY phase call, like fn_step_aux.  bk == NULL: the entry point without _bkgd, launch for launch.
 *   -1 before anything is enqueued, beside the refusals of those entry points: args->white_bkgd != 0 together with bk, a NULL member of
 *   bk that the phases need (bkgd_used, target_ws, g_acc1 and with two passes g_acc0; forward: exactly one of bkgd / seed != 0). */
typedef struct fn_step_bkgd {
  const float* bkgd;                /* [n,3] or NULL: drawn from seed */
  uint64_t seed;
  const float* alpha;               /* [n] or NULL */
  float *bkgd_used, *target_ws;     /* [n,3] each */
  float *g_acc1, *g_acc0;           /* [n] each; g_acc0 unused with one pass */
} fn_step_bkgd;
int64_t fastnerf_step_bkgd_size(void);              /* sizeof(fn_step_bkgd): binding sanity check */
int fastnerf_bkgd_blend(int64_t n, const float* bkgd, uint64_t seed, const float* alpha, const float* acc1, const float* acc0,
                        float* rgb1, float* rgb0, const float* target, float* target_out, float* bkgd_used, fn_stream_t stream);
int fastnerf_bkgd_grad(int64_t n, const float* bkgd_used, const float* g_rgb1, const float* g_rgb0, const float* add1, const float* add0,
                       float* g_acc1, float* g_acc0, fn_stream_t stream);
int fastnerf_train_step_bkgd(const fn_step_args* args, const fn_step_aux* aux, const fn_step_bkgd* bk, int phases, fn_stream_t stream);
int fastnerf_train_step_march_bkgd(const fn_step_args* args, const fn_step_march* march, const fn_step_bkgd* bk, int phases,
                                   fn_stream_t stream);

/* ---- distortion loss on the ray weights (csrc/distortion.hip, render.cpp) ------------------------------------------------------------
 * The regulariser of mip-NeRF 360 (Barron et al. 2022, eq. 15) that pulls the weight of a ray together: it removes floaters and
 * half-transparent fog, which the colour loss alone does not punish.  Per ray, with samples z_0 <= ... <= z_{S-1}, weights w_i >= 0 and
 * near / far = columns 6 / 7 of its rays11 row as the forward left them (tightened bounds and marched rows included):
 *   edges     e_i = z_i (i < S), e_S = max(far, z_{S-1}); interval i is [e_i, e_{i+1}].  In a marched row the interval of live sample b
 *             ends at its closing entry; closing and padding slots carry w = 0.
 *   t(x)      (x - near) / (far - near), or with lindisp (1/near - 1/x) / (1/near - 1/far)
 *   delta_i = t(e_{i+1}) - t(e_i),   m_i = (t(e_i) + t(e_{i+1})) / 2
 *   l       = sum_i sum_j w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 delta_i
 * Differentiable in w only: depths, near and far are constants, as they are everywhere in this renderer.
 *   fastnerf_distortion   w, z [n,S], 1 <= S <= 512.  ell [n] = l; g_w [n,S] = coef * (g_up ? g_up[r] : 1) * dl_r/dw_i.  ell and g_w may
 *                         each be NULL, not both.  A ray whose far - near (with lindisp 1/near - 1/far) is not a positive finite number,
 *                         or whose byte in skip [n] (may be NULL) is non-zero, gets l = +0 and a row of +0.  All-zero weights give +0
 *                         throughout; repeated depths are legal.  One wave per ray, shuffle scans, no atomics: bit-identical from run to
 *                         run.  Nothing cancels (distortion.hip): with the fp32 inputs taken as exact, l and every dl/dw_i have a
 *                         relative error of at most (2 S + 32) 2^-24.  n == 0 returns 0.
 *   fastnerf_distortion_mean  loss2d[0] = mean of ell1 [n], loss2d[1] = mean of ell0 [n] (0 when ell0 == NULL): one workgroup, fixed
 *                         order, fp64, as fastnerf_aux_loss sums; written, not accumulated.
 *   fn_weight_grads       d(loss)/d(weights) of the image pass (g_w1 [n, N_samples + N_importance]; the only pass's [n, N_samples] when
 *                         N_importance == 0) and of the coarse pass of two (g_w0 [n, N_samples]), each may be NULL.
 *   fastnerf_render_rays_bwd_w / _bwd_live_w   the _maps entry points with that struct in front of the stream: a pass whose member is
 *                         set goes through fastnerf_raw2outputs_bwd_full with it as g_w, and counts as a pass with a gradient even
 *                         when it has no other.  wg == NULL: the _maps entry point, launch for launch.
 *   fastnerf_train_step_dist / fastnerf_train_step_march_dist   fastnerf_train_step_bkgd / fastnerf_train_step_march_bkgd (aux and bk may
 *                         be NULL as there) with the term:
 *     FN_STEP_FORWARD  behind the loss launches of the step: fastnerf_distortion on the image pass's (w, z) into ell1 / g_w1 and, with two
 *                      passes, on the coarse pass's into ell0 / g_w0, coef = grad_scale * lambda_dist / n; then fastnerf_distortion_mean
 *                      into loss2d.  The marched step runs it on the packed row with skip = overflow (a truncated row is an artefact of
 *                      the row: fastnerf_march_mask).  The step's loss is loss2[0] + loss2[1] + lambda_dist (loss2d[0] + loss2d[1]) (+
 *                      the other terms).
 *     backward phases  g_w1 / g_w0 go to the compositing backward of their pass (fn_weight_grads).
 *   fn_step_dist is given in EVERY phase call, like fn_step_aux.  dist == NULL or lambda_dist == 0: the entry point without _dist, launch
 *   for launch.  -1 before anything is enqueued, beside the refusals of those entry points: a negative or non-finite lambda_dist, a NULL
 *   member that the phases need (g_w1, ell1, loss2d; with two passes g_w0, ell0), missing weights buffers (w0, w1) in a forward phase.
 *   As with the opacity term, every sample with positive density on a ray that has not saturated receives a gradient and becomes
 *   live: early compacted steps run over more points than without the term. */
typedef struct fn_weight_grads {
  const float *g_w1, *g_w0;
} fn_weight_grads;
typedef struct fn_step_dist {
  float lambda_dist;
  float *ell1, *ell0;               /* [n] each out: the per-ray l of the image pass / the coarse pass of two */
  float *g_w1, *g_w0;               /* [n, S] of their pass, out: coef * dl/dw */
  float* loss2d;                    /* [2] out: the batch means of ell1, ell0 */
} fn_step_dist;
int64_t fastnerf_step_dist_size(void);              /* sizeof(fn_step_dist): binding sanity check */
int fastnerf_distortion(int64_t n, int S, const float* w, const float* z, const float* rays11, int lindisp, const uint8_t* skip,
                        float coef, const float* g_up, float* ell, float* g_w, fn_stream_t stream);
int fastnerf_distortion_mean(int64_t n, const float* ell1, const float* ell0, float* loss2d, fn_stream_t stream);
int fastnerf_render_rays_bwd_w(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11, int white_bkgd,
                               const float* g_rgb, const float* g_rgb0, const float* noise0, const float* noise1, const float* z0,
                               const float* raw0, const float* act0, const float* z1, const float* raw1, const float* act1,
                               const float* params_c, const float* packed_bwd_c, const float* params_f, const float* packed_bwd_f,
                               float* draw_ws, float* dact_ws, float* partial_ws, float* grads_c, float* grads_f, const float* acc0,
                               const float* depth0, const float* acc1, const float* depth1, const fn_map_grads* maps,
                               const fn_weight_grads* wg, fn_stream_t stream);
int fastnerf_render_rays_bwd_live_w(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11, int white_bkgd,
                                    const float* g_rgb, const float* g_rgb0, const float* noise0, const float* noise1, const float* z0,
                                    const float* raw0, const float* z1, const float* raw1, const float* params_c,
                                    const float* packed_fwd_c, const float* packed_bwd_c, const float* params_f,
                                    const float* packed_fwd_f, const float* packed_bwd_f, float* draw_ws, float* act_ws, float* dact_ws,
                                    float* partial_ws, int32_t* live_ws, float* grads_c, float* grads_f, int32_t* counts_out,
                                    const float* acc0, const float* depth0, const float* acc1, const float* depth1,
                                    const fn_map_grads* maps, const fn_weight_grads* wg, fn_stream_t stream);
int fastnerf_train_step_dist(const fn_step_args* args, const fn_step_aux* aux, const fn_step_bkgd* bk, const fn_step_dist* dist,
                             int phases, fn_stream_t stream);
int fastnerf_train_step_march_dist(const fn_step_args* args, const fn_step_march* march, const fn_step_bkgd* bk,
                                   const fn_step_dist* dist, int phases, fn_stream_t stream);

/* ---- density gradient: d(sigma)/d(x) through the fused MLP (csrc/sigma_grad.hip) -------------------------------------------------
 * sigma[n,S] (may be NULL) = raw[..., 3] of the forward of `math_mode` (0 exact fp32, 1 split-bf16 "bf16x3", 2 "bf16x6") at the
 * points o + d*z of fastnerf_mlp_fwd, and grad[n,S,3] = its gradient with respect to the point.  Both are taken BEFORE the ReLU
 * that raw2outputs applies to the logit: where the logit is negative the density is zero and flat, the logit's gradient still
 * points along the field.  One call enqueues the saving forward, a fill of the cotangent (0, 0, 0, 1), the dX chain alone (no dW,
 * no reduction) and one kernel that multiplies the pre-activation gradients of layer 0 and of the skip layer by their input
 * weights and applies the chain rule of the positional encoding with the saved sines and cosines.  No atomics: bit-identical from
 * call to call, and a point's result does not depend on where it sits in the batch.  params / packed_fwd / packed_bwd: the flat
 * parameters and the packed weights of the mode's pack entry point.  ws: fastnerf_mlp_sigma_grad_ws_floats(math_mode, n*S)
 * floats of scratch (saved activations + pre-activation gradients + cotangent and logits of one call, about 20 KB per point).
 * kind 0 only: -1 for kind 1 / 2 (the nerf++ nets), for a math_mode outside 0..2, n <= 0, S <= 0 or a NULL buffer other than
 * sigma, before anything is enqueued.
 * Differentiates model.py:38-63 (NeRF.forward, alpha_linear of the trunk) composed with run_nerf_helpers.py:15-46 (Embedder:
 * [x, sin(2^k x), cos(2^k x)], k = 0..9). */
int64_t fastnerf_mlp_sigma_grad_ws_floats(int math_mode, int64_t n_points);
int fastnerf_mlp_sigma_grad(int math_mode, int kind, int64_t n, int S, const float* rays11, const float* z, const float* params,
                            const float* packed_fwd, const float* packed_bwd, float* ws, float* sigma, float* grad,
                            fn_stream_t stream);

/* ---- ray gradient: d(loss)/d(ray batch) of one pass of render_rays (csrc/ray_grad.hip) -----------------------------------------------
 * d_rays [n,11] = the gradient of a loss with respect to the pass's rays (o, d, near, far, viewdir), given what the pass's backward
 * left behind.  Call it AFTER fastnerf_raw2outputs_bwd (draw [n,S,4] = d(loss)/d(raw)) and the MLP backward of `math_mode` on that draw
 * (fastnerf_mlp_bwd_ex / fastnerf_mlp_x6_bwd), while `dact` (its pre-activation gradients) and `act` (the saving forward's
 * activations) are still valid: with g[p] = d(loss)/d(point p) = the kernel of fastnerf_mlp_sigma_grad run on dact's dY0 / dY5,
 *   d_o[r] = sum_s g[r,s]
 *   d_d[r] = sum_s z[r,s] g[r,s] + c_r d_r / |d_r|^2,   c_r = sum_s draw[r,s,3] (raw[r,s,3] + noise[r,s])
 *            (the second term: dists = dz |d| in raw2outputs, render.py:167; 0 for a ray with d = 0)
 *   d_viewdir[r] = the PE(4) chain rule on (sum_s dYv[r,s]) Wv[:, 256:283], with the saved sines and cosines
 *   columns 6:8 (near, far) = 0: z is a constant of the pass (render.py:244-266 and the detach of render.py:281), near / far are
 *   not differentiated.
 * This is autograd of render.py:195-305 for one pass with respect to ray_batch.  z, raw, noise (NULL = none), rays11: the inputs
 * of the pass's fastnerf_raw2outputs_bwd.  params: the flat parameters.  ws: fastnerf_ray_grad_ws_floats(math_mode, n, S) floats of
 * scratch (g).  accumulate != 0 adds to d_rays (a second pass on top of the first), 0 overwrites its n rows.  No atomics: bit-identical
 * from call to call, and a ray's result does not depend on where it sits in the batch.
 * -1 before anything is enqueued: math_mode outside 0..2, n < 0, S < 1; kind != 0 (the nerf++ nets); math_mode 1 (bf16x3: its
 * K-fragment tensors have no ray-gradient kernel); a NULL buffer other than noise when n > 0.  n == 0 returns 0 at once. */
int64_t fastnerf_ray_grad_ws_floats(int math_mode, int64_t n, int S);
int fastnerf_ray_grad(int math_mode, int kind, int64_t n, int S, const float* rays11, const float* z, const float* raw,
                      const float* noise, const float* draw, const float* act, const float* dact, const float* params, float* ws,
                      int accumulate, float* d_rays, fn_stream_t stream);

/* ---- pose table: camera poses that training refines (csrc/pose.hip) ------------------------------------------------------------------
 * Per image i a 6-vector xi_i = (omega_i, tau_i) beside a fixed base pose (R0_i | t0_i), all poses row-major 3x4 camera-to-world:
 *   R_i = exp(hat(omega_i)) R0_i,   t_i = t0_i + tau_i
 * (the camera turns about its own centre, in world axes, and moves independently).  Rays are the pinhole rays of
 * fastnerf_gen_rays_pixels + fastnerf_pack_rays with ndc = 0:  dir = ((col - cx) / fx, -(row - cy) / fy, -1),  o = t,  d = R dir,
 * v = d / |d|.
 *
 * fastnerf_pose_exp: poses_out [n_img,3,4] from base [n_img,3,4] and xi [n_img,6], one lane per image.  Rodrigues,
 *   exp(hat(w)) = I + a K + b K^2,  K = hat(w),  a = sin(th) / th,  b = 1/2 (sin(th/2) / (th/2))^2,  th = |w|
 * (b in the half-angle form, in which nothing cancels; a and b by series below th = 1e-3, so a(0) = 1 and b(0) = 1/2 exactly and
 * nothing divides by zero).  xi == NULL, or an image whose omega is zero, returns that image's base rotation BIT FOR BIT, a zero
 * component of tau that component of t0 bit for bit; every other t is the fp32 sum t0 + tau.
 *
 * fastnerf_pose_exp_bwd: d_xi [n_img,6] from d_poses [n_img,3,4] = d(loss)/d(poses_out):
 *   d_tau   = column 3 of d_poses, copied
 *   d_omega = J_l(omega)^T sum_k (A_k x G_k),   A = R R0 (rebuilt), G = d_poses[:, :, :3], both column by column,
 *   J_l = I + b K + c K^2,   c = (th - sin(th)) / th^3   (by series below th = 0.5, where the difference would cancel)
 * This is autograd of the matrix exponential composed with R0, at th = 0 too (J_l = I).
 *
 * fastnerf_pose_grad: d_poses [n_img,3,4] = the gradient of a loss with respect to the poses, given d_rays [n,11] = d(loss)/d(ray
 * batch) (fastnerf_ray_grad) of the rays that pix [n,3] = (image, row, col) names; d and v are rebuilt from poses and pix:
 *   g_d = d_d + (d_v - v (v . d_v)) / |d|
 *   d_poses[img, j, k] = sum over the rays of img of g_d[j] dir[k]   (k < 3),     d_poses[img, j, 3] = sum of d_o[j]
 * Columns 6:8 of d_rays are ignored; a batch without view directions has zeros in 8:11.  pix rows must name existing images, as for
 * fastnerf_gen_rays_pixels.  A segmented sum without atomics: a ray's place in the sum depends on its row index alone, so the
 * result is bit-identical from call to call; an image without a ray in the batch gets twelve +0, written; n == 0 writes n_img * 12
 * zeros (when d_poses is given) and returns 0.  Any n: the batch is walked in chunks, never one thread per ray of a capped grid.
 * ws: fastnerf_pose_grad_ws_floats(n, n_img) floats of scratch (0 for a small batch: NULL is then accepted).
 *
 * -1 before anything is enqueued: n_img < 1; n < 0; a NULL buffer other than xi (pose_grad: when n > 0; ws only when its size is
 * not 0).  All stores are plain vector stores. */
int fastnerf_pose_exp(int n_img, const float* base, const float* xi, float* poses_out, fn_stream_t stream);
int fastnerf_pose_exp_bwd(int n_img, const float* base, const float* xi, const float* d_poses, float* d_xi, fn_stream_t stream);
int64_t fastnerf_pose_grad_ws_floats(int64_t n, int n_img);
int fastnerf_pose_grad(int64_t n, int n_img, const int32_t* pix, const float* poses, float fx, float fy, float cx, float cy,
                       const float* d_rays, float* ws, float* d_poses, fn_stream_t stream);

/* ---- exposure table: per-image exposures that training fits beside the field (csrc/exposure.hip) -------------------------------------
 * Per image i a row ab[i] = (a_i, shift_i) of ab [n_img,2]; scale_i = |a_i| + 0.5, so that the row (0.5, 0) is the identity (the
 * reference's autoexposure parameters, nerf++-ours ddp_model.py:157-188).  img [n] int32 names the image of every ray.  For ray r of
 * image i = img[r], per pass p (1: the pass that produces the image, 0: the coarse pass of two) and channel c:
 *   e_p[r,c] = (rgb_p[r,c] - shift_i) / scale_i              one fsub, one IEEE division; rgb_p behind the background blend
 *   L = mse(e_1, t) + mse(e_0, t) + lambda (1/n) sum_r (|scale_i(r) - 1| + |shift_i(r)|)
 * (for a batch drawn from one image, the reference's loss).
 *
 * fastnerf_expo_apply: e1 / e0 [n,3] from rgb1 / rgb0 [n,3]; rgb0 and e0 are NULL with one pass.  One thread per ray.
 *
 * fastnerf_expo_grad: with G_p = dL/de_p in g1 / g0 [n,3] (what fastnerf_mse_leafmax leaves, grad_scale included),
 *   g_p[r,c]  = G_p[r,c] / scale_i                           written over G_p IN PLACE: the colour gradient every later launch reads
 *   d_shift_i = -sum_{r in i} sum_{p,c} g_p[r,c],     d_scale_i = -sum_{r in i} sum_{p,c} g_p[r,c] e_p[r,c]
 *   d_ab[i,0] = sign(a_i) (d_scale_i + lambda grad_scale cnt_i/n sign(scale_i - 1))           sign(0) = 0, as torch.abs differentiates
 *   d_ab[i,1] = d_shift_i + lambda grad_scale cnt_i/n sign(shift_i)
 *   counts[i] = cnt_i, the number of rays of image i;   loss_reg[0] = sum_i (cnt_i/n) (|scale_i - 1| + |shift_i|), images in index order
 * d_ab [n_img,2], counts [n_img] int32 and loss_reg [1] are written, not accumulated; an image without a ray gets an exact zero row.
 * A segmented sum without atomics (the scheme of fastnerf_pose_grad): workgroup (image, chunk) walks a contiguous chunk of the batch
 * and owns the rays of it that name its image, lane sums in ray order, a fixed tree over the 256 lanes, the chunks in chunk order in a
 * finish launch; the chunk count is a function of (n, n_img) alone: bit-identical from call to call.  n == 0: the finish launch alone
 * writes zeros.  ws: fastnerf_expo_grad_ws_floats(n, n_img) floats of scratch (0 only for n == 0).
 *
 * A ray whose img lies outside [0, n_img) is left untouched by both (e = rgb, g = G) and belongs to no image: the kernels read no
 * table row for it.  With the identity row e has the bits of rgb and g those of G.
 *
 * -1 before anything is enqueued: n < 0 or n >= 2^31; n_img < 1; a negative or non-finite lambda; a NULL table or output; with n > 0 a
 * NULL img, map, gradient or ws; rgb0 / e0 (apply) or e0 / g0 (grad) not both set or both NULL.  All stores are plain vector stores.
 *
 * fastnerf_train_step_expo / fastnerf_train_step_march_expo: fastnerf_train_step_dist / fastnerf_train_step_march_dist (aux, bk and dist
 * may be NULL as there) with the term.  FN_STEP_FORWARD: the loss launches become  blend -> expo_apply -> mse_leafmax on e1 / e0 ->
 * depth / opacity terms -> march mask -> expo_grad on g_rgb / g_rgb0 -> bkgd_grad -> distortion.  The leaf-error table sees e; rgb0 /
 * rgb1 stay the scene's colours.  An overflowed marched ray has G = 0 and gives the table nothing, but counts in cnt.  The step's loss is
 * loss2[0] + loss2[1] + lambda loss_reg[0] (+ the other terms).  fn_step_expo is read in a forward phase only.  ex == NULL: the _dist
 * entry point, launch for launch.  -1 before anything is enqueued, beside the refusals of those entry points: n_img < 1, a negative or
 * non-finite lambda, n >= 2^31, a NULL member in a forward phase (e0 with two passes only). */
typedef struct fn_step_expo {
  const int32_t* img;               /* [n] */
  const float* ab;                  /* [n_img,2] */
  int n_img;
  float lambda;
  float *e1, *e0;                   /* [n,3] each out: what the colour loss saw (e0 with two passes) */
  float* ws;                        /* fastnerf_expo_grad_ws_floats(n, n_img) floats */
  float* d_ab;                      /* [n_img,2] out */
  int32_t* counts;                  /* [n_img] out */
  float* loss_reg;                  /* [1] out */
} fn_step_expo;
int64_t fastnerf_step_expo_size(void);              /* sizeof(fn_step_expo): binding sanity check */
int fastnerf_expo_apply(int64_t n, int n_img, const int32_t* img, const float* ab, const float* rgb1, const float* rgb0, float* e1,
                        float* e0, fn_stream_t stream);
int64_t fastnerf_expo_grad_ws_floats(int64_t n, int n_img);
int fastnerf_expo_grad(int64_t n, int n_img, const int32_t* img, const float* ab, float lambda, float grad_scale, const float* e1,
                       const float* e0, float* g1, float* g0, float* ws, float* d_ab, int32_t* counts, float* loss_reg,
                       fn_stream_t stream);
int fastnerf_train_step_expo(const fn_step_args* args, const fn_step_aux* aux, const fn_step_bkgd* bk, const fn_step_dist* dist,
                             const fn_step_expo* ex, int phases, fn_stream_t stream);
int fastnerf_train_step_march_expo(const fn_step_args* args, const fn_step_march* march, const fn_step_bkgd* bk,
                                   const fn_step_dist* dist, const fn_step_expo* ex, int phases, fn_stream_t stream);
/* The two steps through an occupancy CASCADE: fastnerf_train_step_expo / fastnerf_train_step_march_expo with the cascade as one more
 * trailing pointer; fn_step_args keeps its size.  cascade == NULL is exactly that call.  cascade != NULL needs args->occ == NULL (-1
 * before anything is enqueued otherwise, as for a level that fails the checks of fastnerf_occ_query_cascade), and each place where the
 * step reads args->occ takes the cascade's twin, which shares its body: fastnerf_occ_ray_bounds (FN_STEP_TIGHTEN),
 * fastnerf_render_rays_fwd_occ_cascade, the check of the descriptor, fastnerf_occ_march_jitter.  Every refusal of the grid's route
 * holds: the compacted step only (live != 0), no sigma noise, live_ws; FN_STEP_TIGHTEN needs one of the two.  A cascade of one level
 * is the step through that grid, bit for bit. */
int fastnerf_train_step_cascade(const fn_step_args* args, const fn_step_aux* aux, const fn_step_bkgd* bk, const fn_step_dist* dist,
                                const fn_step_expo* ex, const fn_occ_cascade* cascade, int phases, fn_stream_t stream);
int fastnerf_train_step_march_cascade(const fn_step_args* args, const fn_step_march* march, const fn_step_bkgd* bk,
                                      const fn_step_dist* dist, const fn_step_expo* ex, const fn_occ_cascade* cascade, int phases,
                                      fn_stream_t stream);

/* ---- environment map: a trained background behind every ray (csrc/envmap.hip) ----------------------------------------------------------
 * A table of colours indexed by ray direction alone, composited behind the volume as rgb += (1 - acc) env(d) through the per-ray
 * background colours above, and trained beside the field.  The map is octahedral: one square table T [R,R,3] fp32 (row j = y, column
 * i = x), 2 <= R <= 16384.  Only + - * / and comparisons; every operation below is rounded on its own (no contraction, one IEEE
 * division), so a float32 restatement matches bit for bit.  For a direction d = (dx, dy, dz) of ANY length:
 *   s = (|dx| + |dy|) + |dz|;   s zero or not finite: p = (0, 0);   otherwise px = dx / s, py = dy / s
 *   dz < 0:  (px, py) = ((1 - |py|) sg(px), (1 - |px|) sg(py)),  sg(t) = t >= 0 ? 1 : -1  (-0 gives +1; both sides use the old px, py)
 *   x = ((px * 0.5 + 0.5) * (float)R) - 0.5,  i0 = floor(x),  fx = x - i0;   y, j0, fy alike from py
 *   neighbours (i0, j0), (i0+1, j0), (i0, j0+1), (i0+1, j0+1), each through the mirror wrap -- the octahedral map's own identification of
 *   its border, so the map has no seam: oi = i outside [0,R), oj = j outside [0,R); clamp both; oi: j = R-1-j; oj: i = R-1-i
 *   w00 = (1-fx)(1-fy), w10 = fx (1-fy), w01 = (1-fx) fy, w11 = fx fy
 *   colour[c] = (w00 T00[c] + w10 T10[c]) + (w01 T01[c] + w11 T11[c])
 *
 * fastnerf_env_lookup: out [n,3] from dirs, read as dirs[r*stride + 0..2] (columns 3:6 of an [n,11] batch are read in place with
 * stride 11).  One thread per ray in a walk of the whole batch (any n), plain stores.
 *
 * fastnerf_env_grad: d_table [R,R,3] (written, not accumulated) from the step's colour gradients and opacity maps; g_rgb0 and acc0 are
 * NULL with one pass.  Per ray and channel
 *   g = (1 - acc1[r]) g_rgb1[r,c] + (1 - acc0[r]) g_rgb0[r,c]
 * and the four terms w_k g go to their texels.  Every term is rounded once, q = llrint((double)term * 2^50), and added with a 64-bit
 * integer vector atomic into ws [R*R*3] int64 (fastnerf_env_grad_ws_bytes(R) bytes, 8-byte aligned, zeroed by the call); a finishing
 * launch writes d_table[t] = (float)((double)ws[t] * 2^-50).  Integer addition is associative: the bits do not depend on arrival order,
 * on the order of the rays, or on how a batch is split; the sum is exact while a texel's sum stays below 2^13.  Non-finite gradients
 * are out of contract.  Directions get no gradient.
 *
 * -1 before anything is enqueued: R < 2 or R > 16384; n < 0; stride < 3; with n > 0 a NULL buffer; a NULL d_table; g_rgb0 and acc0 not
 * both set or both NULL.  n == 0: the lookup returns 0 at once, the gradient writes R*R*3 zeros. */
int fastnerf_env_lookup(int64_t n, const float* dirs, int64_t stride, const float* table, int R, float* out, fn_stream_t stream);
int64_t fastnerf_env_grad_ws_bytes(int R);
int fastnerf_env_grad(int64_t n, const float* dirs, int64_t stride, int R, const float* g_rgb1, const float* acc1, const float* g_rgb0,
                      const float* acc0, void* ws, float* d_table, fn_stream_t stream);

/* ---- band weights: a weight per column of the positional encodings, for coarse-to-fine training (csrc/bands.hip) ------------------------
 * A weighted encoding w (.) gamma(x) enters a network through three matrices only -- layer 0, the skip layer and the view layer -- and
 * W (w (.) gamma) = (W diag(w)) gamma.  So every MLP kernel runs, unchanged, on an EFFECTIVE network whose encoding columns are the
 * master's times w, and the master's gradient is the effective network's with the same columns times w.  The three regions of a net of
 * layout `kind` (offsets of csrc/mlp_layout.h, [out][in] row-major): LW[0][:, 0:in_pe] and LW[5][:, 0:in_pe] take w_pos[col], in_pe = 63
 * (84 for kind 2) floats; VW[:, 256:283] takes w_view[col - 256], 27 floats.
 *
 * fastnerf_band_apply: effective[e] = master[e] for every float of the net, copied bit for bit without a multiply, except in the three
 * regions, where effective[e] = master[e] * w[col], one fp32 multiply.  One grid-stride launch over the net's floats.
 *
 * fastnerf_band_grad: in place, the three regions of a gradient buffer times w[col]; no other float is read or written.
 *
 * -1 before anything is enqueued: a kind outside 0..2, a NULL pointer, master == effective. */
int fastnerf_band_apply(int kind, const float* w_pos, const float* w_view, const float* master, float* effective, fn_stream_t stream);
int fastnerf_band_grad(int kind, const float* w_pos, const float* w_view, float* grads, fn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
