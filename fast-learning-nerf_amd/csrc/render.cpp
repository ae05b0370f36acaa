// render.cpp -- host-side sequencing of the fused forward of render_rays (render.py:238-299): one C-ABI call
// enqueues  coarse sampler -> coarse MLP -> compositing -> [inverse-CDF + merge -> fine MLP -> compositing]
// on the caller's stream.  No kernels here; every stage is one of the library's own entry points.  The chain is written once
// (rr_fwd_chain) and every MLP call goes through one table of entry points indexed by the math mode (modes[]).  Likewise the marched
// round (march_round: the marched render's rounds and the marched step's forward), the backward -- a pass is a value (BwdPass), resolved
// from the flat argument lists in one place (bwd_passes) and run by rr_bwd / rr_bwd_live -- and the stages the two optimisation steps
// share (step_pack_rays, step_list_ok, step_update).
#include <stdint.h>
#include "../../include/fastnerf.h"
#include "dw_pair.h"
#include "host_state.h"   // fn::stream_ws: the marched render's scratch

namespace fn {
void set_error(const char* fmt, ...);
const char* occ_cascade_fault(const fn_occ_cascade* c);   // occupancy.hip
const char* occ_grid_fault(const fn_occ_grid* g);         // occupancy.hip
// mlp_bwd_dw.hip, the paired bf16x6 backward: workspace -> the side dact / partial set of this (device, stream) for the coarse pass, or false (a stream
// capture, no memory: take the unpaired route); pass -> everything of fastnerf_mlp_x6_bwd but the trunk launch, the reduction and the unfold, which
// it records in *d; finish -> ONE trunk launch over both passes, then each net's reduction and unfold
bool x6_pair_workspace(int64_t P_coarse, fn_stream_t stream, float** dact2, float** partial2);
// rb != NULL: the pass's view job rebuilds dYv from hv, draw and Wr, and dX does not store it (dw_pair.h SideRb);
// x6_bwd_rebuild: a whole unpaired pass of that kind;  side_rebuild_mode: FASTNERF_SIDE_REBUILD, 0 off / 1 on / 2 on with dact_yv poisoned
int x6_pair_pass(DwDeferred* d, int64_t n, int S, const float* draw, const float* act, const float* params, const float* packed_bwd,
                 float* dact, float* partial, float* grads, fn_stream_t stream, const SideRb* rb);
int x6_pair_finish(const DwDeferred* fine, const DwDeferred* coarse, fn_stream_t stream);
int x6_bwd_rebuild(int64_t n, int S, const float* draw, const float* act, const float* params, const float* packed_bwd, float* dact,
                   float* partial, float* grads, fn_stream_t stream, const SideRb* rb);
int side_rebuild_mode(void);
}

// ---- the math modes: one row of MLP entry points per math_mode (0 exact fp32, 1 split-bf16 "bf16x3", 2 "bf16x6") -----------------
// A further mode is a further row.  The three families have one signature per operation except the plain forward, where only
// fastnerf_mlp_x6_fwd takes both `act` and `flags`: the other two get an adapter with that signature.
struct MlpMode {
  int (*pack)(int kind, const float* params, float* packed_fwd, float* packed_bwd, fn_stream_t);
  int (*fwd)(int kind, int64_t n, int S, const float* rays11, const float* z, const float* params, const float* packed_fwd, float* raw,
             float* act, int flags, fn_stream_t);
  int (*fwd_list)(int kind, int64_t n, int S, const float* rays11, const float* z, const float* params, const float* packed_fwd,
                  float* raw, const int32_t* live_idx, const int32_t* live_cnt, int flags, fn_stream_t);
  int (*fwd_live)(int kind, int64_t n, int S, const float* rays11, const float* z, const float* params, const float* packed_fwd,
                  float* act, const int32_t* live_idx, const int32_t* live_cnt, fn_stream_t);
  int (*bwd)(int kind, int64_t n, int S, const float* draw, const float* act, const float* params, const float* packed_bwd, float* dact,
             float* partial, float* grads, fn_stream_t);
  int (*bwd_live)(int kind, int64_t n, int S, const float* draw, const float* act, const float* params, const float* packed_bwd,
                  float* dact, float* partial, float* grads, const int32_t* live_idx, const int32_t* live_cnt, fn_stream_t);
};

// a training launch (act != NULL) has no options; an inference launch with flags == 0 is the plain forward with act == NULL
static int fwd_fp32(int kind, int64_t n, int S, const float* rays11, const float* z, const float* params, const float* packed_fwd,
                    float* raw, float* act, int flags, fn_stream_t stream) {
  return act ? fastnerf_mlp_fwd_ex(kind, n, S, rays11, z, params, packed_fwd, raw, act, stream)
             : fastnerf_mlp_fwd_flags_ex(kind, n, S, rays11, z, params, packed_fwd, raw, flags, stream);
}

static int fwd_bf16(int kind, int64_t n, int S, const float* rays11, const float* z, const float* params, const float* packed_fwd,
                    float* raw, float* act, int flags, fn_stream_t stream) {
  return act ? fastnerf_mlp_bf16_fwd(kind, n, S, rays11, z, params, packed_fwd, raw, act, stream)
             : fastnerf_mlp_bf16_fwd_flags(kind, n, S, rays11, z, params, packed_fwd, raw, flags, stream);
}

static const MlpMode modes[3] = {
    {fastnerf_mlp_pack_ex, fwd_fp32, fastnerf_mlp_fwd_list_ex, fastnerf_mlp_fwd_live_ex, fastnerf_mlp_bwd_ex, fastnerf_mlp_bwd_live_ex},
    {fastnerf_mlp_bf16_pack, fwd_bf16, fastnerf_mlp_bf16_fwd_list, fastnerf_mlp_bf16_fwd_live, fastnerf_mlp_bf16_bwd,
     fastnerf_mlp_bf16_bwd_live},
    {fastnerf_mlp_x6_pack, fastnerf_mlp_x6_fwd, fastnerf_mlp_x6_fwd_list, fastnerf_mlp_x6_fwd_live, fastnerf_mlp_x6_bwd,
     fastnerf_mlp_x6_bwd_live},
};

// ---- the forward ------------------------------------------------------------------------------------------------------------
// What the forward entry points share: `fname` names the caller in the error texts, noise0 / noise1 are NULL through a grid.
struct RrFwd {
  const char* fname;
  int math_mode;
  int64_t n;
  int N_samples, N_importance;
  const float* rays11;
  int lindisp, perturb, det, white_bkgd;
  const float *t_rand, *u, *noise0, *noise1;
  uint64_t seed0, seed1;
  const float *params_c, *packed_c, *params_f, *packed_f;
  float *z0, *raw0, *rgb0, *disp0, *acc0, *w0, *depth0, *z1, *z_samples, *z_std, *raw1, *rgb1, *disp1, *acc1, *w1, *depth1;
  int flags;
  fn_stream_t stream;
};

// the checks that come before the n == 0 return
static bool rr_fwd_scalars(const RrFwd& a) {
  if (a.math_mode < 0 || a.math_mode > 2 || a.n < 0 || a.N_samples < 2 || a.N_importance < 0) {
    fn::set_error("%s: bad argument: math_mode in {0,1,2}, n>=0, N_samples>=2, N_importance>=0", a.fname);
    return false;
  }
  if (a.N_importance > 0 && a.N_samples < 3) {
    // the reference fails here too: weights[..., 1:-1] is empty and sample_pdf indexes an empty cdf (run_nerf_helpers.py:147)
    fn::set_error("%s: hierarchical sampling needs N_samples >= 3 (the inner weights of 2 samples are empty)", a.fname);
    return false;
  }
  return true;
}

static bool rr_fwd_coarse_ptrs(const RrFwd& a) {
  return a.rays11 && a.params_c && a.packed_c && a.z0 && a.raw0 && a.rgb0 && a.disp0 && a.acc0 && a.w0 && a.depth0;
}

// The chain, once: sampler -> net -> compositing [-> inverse-CDF + merge -> net -> compositing].  net(pass, S, z, params, packed,
// raw, noise) enqueues whatever fills raw [n, S, 4] for pass 0 (coarse) / 1 (fine); the caller has made the checks up to the
// coarse pass.
template <class Net>
static int rr_fwd_chain(const RrFwd& a, Net&& net) {
  int rc;
  if ((rc = fastnerf_sample_coarse(a.n, a.N_samples, a.rays11, a.lindisp, a.perturb, a.t_rand, a.seed0, a.z0, a.stream))) return rc;
  if ((rc = net(0, a.N_samples, a.z0, a.params_c, a.packed_c, a.raw0, a.noise0))) return rc;
  if ((rc = fastnerf_raw2outputs_fwd(a.n, a.N_samples, a.raw0, a.z0, a.rays11, a.noise0, a.white_bkgd, a.rgb0, a.disp0, a.acc0, a.w0,
                                     a.depth0, a.stream)))
    return rc;
  if (a.N_importance == 0) return 0;
  if (!a.params_f || !a.packed_f || !a.z1 || !a.z_samples || !a.z_std || !a.raw1 || !a.rgb1 || !a.disp1 || !a.acc1 || !a.w1 ||
      !a.depth1) {
    fn::set_error("%s: null pointer (fine pass)", a.fname);
    return -1;
  }
  const int S1 = a.N_samples + a.N_importance;
  if ((rc = fastnerf_sample_pdf_merge(a.n, a.N_samples, a.N_importance, a.z0, a.w0, a.det, a.u, a.seed1, a.z1, a.z_samples, a.z_std,
                                      a.stream)))
    return rc;
  if ((rc = net(1, S1, a.z1, a.params_f, a.packed_f, a.raw1, a.noise1))) return rc;
  return fastnerf_raw2outputs_fwd(a.n, S1, a.raw1, a.z1, a.rays11, a.noise1, a.white_bkgd, a.rgb1, a.disp1, a.acc1, a.w1, a.depth1,
                                  a.stream);
}

extern "C" int fastnerf_render_rays_fwd_ex(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11,
                                        int lindisp, int perturb, int det, int white_bkgd, const float* t_rand, const float* u,
                                        const float* noise0, const float* noise1, uint64_t seed0, uint64_t seed1,
                                        const float* params_c, const float* packed_c, const float* params_f,
                                        const float* packed_f, float* z0, float* raw0, float* act0, float* rgb0,
                                        float* disp0, float* acc0, float* w0, float* depth0, float* z1,
                                        float* z_samples, float* z_std, float* raw1, float* act1, float* rgb1,
                                        float* disp1, float* acc1, float* w1, float* depth1, int flags, fn_stream_t stream) {
  const RrFwd a = {"fastnerf_render_rays_fwd", math_mode, n, N_samples, N_importance, rays11, lindisp, perturb, det, white_bkgd, t_rand,
                   u, noise0, noise1, seed0, seed1, params_c, packed_c, params_f, packed_f, z0, raw0, rgb0, disp0, acc0, w0, depth0, z1,
                   z_samples, z_std, raw1, rgb1, disp1, acc1, w1, depth1, flags, stream};
  if (!rr_fwd_scalars(a)) return -1;
  if (n == 0) return 0;
  if (!rr_fwd_coarse_ptrs(a)) {
    fn::set_error("%s: null pointer (coarse pass)", a.fname);
    return -1;
  }
  // (options only where their precondition holds: an inference launch, no sigma noise in that pass)
  return rr_fwd_chain(a, [&](int pass, int S, const float* z, const float* params, const float* packed, float* raw, const float* noise) {
    float* act = pass ? act1 : act0;
    return modes[math_mode].fwd(0, n, S, rays11, z, params, packed, raw, act, (!act && !noise) ? flags : 0, stream);
  });
}

// The same chain through an occupancy grid or a cascade of them (inference): per pass, the samples are sorted by it
// (fastnerf_occ_classify / _cascade: list of the occupied ones, zero logits for the others) and the network runs over the list only.
// One body for both entry points: exactly one of grid / cascade is set.  counts_out: (occupied, total) coarse, then fine.
static int rr_fwd_occ(const RrFwd& a, const fn_occ_grid* grid, const fn_occ_cascade* cascade, int32_t* live_ws, int32_t* counts_out) {
  if (!rr_fwd_scalars(a)) return -1;
  if (a.n == 0) return 0;
  const int64_t P1 = a.n * (int64_t)(a.N_samples + a.N_importance);
  if (P1 >= ((int64_t)1 << 31)) {
    fn::set_error("%s: bad argument: n * (N_samples + N_importance) < 2^31 (lists index points with int32)", a.fname);
    return -1;
  }
  if (!rr_fwd_coarse_ptrs(a) || (!grid && !cascade) || !live_ws || !counts_out) {
    fn::set_error("%s: null pointer (coarse pass)", a.fname);
    return -1;
  }
  if (const char* fault = cascade ? fn::occ_cascade_fault(cascade) : nullptr) {   // before anything is enqueued
    fn::set_error("%s: bad argument: %s", a.fname, fault);
    return -1;
  }
  int32_t* idx = live_ws;
  int32_t* cws = live_ws + P1;
  return rr_fwd_chain(a, [&](int pass, int S, const float* z, const float* params, const float* packed, float* raw, const float*) {
    int32_t* cnt = counts_out + 2 * pass;
    if (int rc = cascade ? fastnerf_occ_classify_cascade(cascade, a.n, S, a.rays11, z, idx, cnt, raw, cws, a.stream)
                         : fastnerf_occ_classify(grid, a.n, S, a.rays11, z, idx, cnt, raw, cws, a.stream))
      return rc;
    return modes[a.math_mode].fwd_list(0, a.n, S, a.rays11, z, params, packed, raw, idx, cnt, a.flags, a.stream);
  });
}

extern "C" int fastnerf_render_rays_fwd_occ(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11, int lindisp,
                                            int perturb, int det, int white_bkgd, const float* t_rand, const float* u, uint64_t seed0,
                                            uint64_t seed1, const float* params_c, const float* packed_c, const float* params_f,
                                            const float* packed_f, const fn_occ_grid* grid, int32_t* live_ws, int32_t* counts_out,
                                            float* z0, float* raw0, float* rgb0, float* disp0, float* acc0, float* w0, float* depth0,
                                            float* z1, float* z_samples, float* z_std, float* raw1, float* rgb1, float* disp1,
                                            float* acc1, float* w1, float* depth1, int flags, fn_stream_t stream) {
  return rr_fwd_occ({"fastnerf_render_rays_fwd_occ", math_mode, n, N_samples, N_importance, rays11, lindisp, perturb, det, white_bkgd,
                     t_rand, u, nullptr, nullptr, seed0, seed1, params_c, packed_c, params_f, packed_f, z0, raw0, rgb0, disp0, acc0, w0,
                     depth0, z1, z_samples, z_std, raw1, rgb1, disp1, acc1, w1, depth1, flags, stream},
                    grid, nullptr, live_ws, counts_out);
}

extern "C" int fastnerf_render_rays_fwd_occ_cascade(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11,
                                                    int lindisp, int perturb, int det, int white_bkgd, const float* t_rand,
                                                    const float* u, uint64_t seed0, uint64_t seed1, const float* params_c,
                                                    const float* packed_c, const float* params_f, const float* packed_f,
                                                    const fn_occ_cascade* cascade, int32_t* live_ws, int32_t* counts_out, float* z0,
                                                    float* raw0, float* rgb0, float* disp0, float* acc0, float* w0, float* depth0,
                                                    float* z1, float* z_samples, float* z_std, float* raw1, float* rgb1, float* disp1,
                                                    float* acc1, float* w1, float* depth1, int flags, fn_stream_t stream) {
  return rr_fwd_occ({"fastnerf_render_rays_fwd_occ_cascade", math_mode, n, N_samples, N_importance, rays11, lindisp, perturb, det,
                     white_bkgd, t_rand, u, nullptr, nullptr, seed0, seed1, params_c, packed_c, params_f, packed_f, z0, raw0, rgb0,
                     disp0, acc0, w0, depth0, z1, z_samples, z_std, raw1, rgb1, disp1, acc1, w1, depth1, flags, stream},
                    nullptr, cascade, live_ws, counts_out);
}

// The same chain with early ray termination in the pass that produces the image (include/fastnerf.h, "early ray termination"): the
// coarse pass of two runs exactly as it does without it (plain, or through the grid / cascade); the image pass runs segment by
// segment: fastnerf_ert_classify (T > eps AND the grid) -> the list forward -> fastnerf_ert_advance (T *= the segment's product, the
// pass's counters += the list length).  live_ws: list | scan scratch | the segment's (count, entries).
extern "C" int fastnerf_render_rays_fwd_ert(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11, int lindisp,
                                            int perturb, int det, int white_bkgd, const float* t_rand, const float* u, uint64_t seed0,
                                            uint64_t seed1, const float* params_c, const float* packed_c, const float* params_f,
                                            const float* packed_f, const fn_occ_grid* grid, const fn_occ_cascade* cascade, float eps,
                                            int block, float* trans_ws, int32_t* live_ws, int32_t* counts_out, float* z0, float* raw0,
                                            float* rgb0, float* disp0, float* acc0, float* w0, float* depth0, float* z1,
                                            float* z_samples, float* z_std, float* raw1, float* rgb1, float* disp1, float* acc1,
                                            float* w1, float* depth1, int flags, fn_stream_t stream) {
  const RrFwd a = {"fastnerf_render_rays_fwd_ert", math_mode, n, N_samples, N_importance, rays11, lindisp, perturb, det, white_bkgd,
                   t_rand, u, nullptr, nullptr, seed0, seed1, params_c, packed_c, params_f, packed_f, z0, raw0, rgb0, disp0, acc0, w0,
                   depth0, z1, z_samples, z_std, raw1, rgb1, disp1, acc1, w1, depth1, flags, stream};
  if (!rr_fwd_scalars(a)) return -1;
  if (!(eps >= 0.f && eps < 1.f) || block < 1) {
    fn::set_error("%s: bad argument: 0 <= eps < 1, block >= 1", a.fname);
    return -1;
  }
  if (grid && cascade) {
    fn::set_error("%s: bad argument: at most one of grid / cascade", a.fname);
    return -1;
  }
  if (n == 0) return 0;
  const int S_img = N_samples + N_importance;
  const int64_t P1 = n * (int64_t)S_img;
  if (P1 >= ((int64_t)1 << 31) || S_img > 512) {
    fn::set_error("%s: bad argument: n * (N_samples + N_importance) < 2^31 (lists index points with int32), at most 512 samples per ray", a.fname);
    return -1;
  }
  if (!rr_fwd_coarse_ptrs(a) || !trans_ws || !live_ws || !counts_out) {
    fn::set_error("%s: null pointer (coarse pass)", a.fname);
    return -1;
  }
  if (N_importance > 0 && (!params_f || !packed_f || !z1 || !z_samples || !z_std || !raw1 || !rgb1 || !disp1 || !acc1 || !w1 || !depth1)) {
    fn::set_error("%s: null pointer (fine pass)", a.fname);
    return -1;
  }
  if (const char* fault = cascade ? fn::occ_cascade_fault(cascade) : (grid ? fn::occ_grid_fault(grid) : nullptr)) {   // before anything is enqueued
    fn::set_error("%s: bad argument: %s", a.fname, fault);
    return -1;
  }
  int32_t* idx = live_ws;
  int32_t* cws = live_ws + P1;
  int32_t* seg = cws + fastnerf_compact_ws_ints(P1);
  const int img = N_importance > 0 ? 1 : 0;
  return rr_fwd_chain(a, [&](int pass, int S, const float* z, const float* params, const float* packed, float* raw, const float*) {
    int32_t* cnt = counts_out + 2 * pass;
    int rc;
    if (pass != img) {   // the coarse pass of two: as without ert
      // (plain: every sample is evaluated, the host knows the pair (n * S, n * S) and nothing is written to it)
      if (!grid && !cascade) return modes[math_mode].fwd(0, n, S, rays11, z, params, packed, raw, nullptr, flags, stream);
      if ((rc = cascade ? fastnerf_occ_classify_cascade(cascade, n, S, rays11, z, idx, cnt, raw, cws, stream)
                        : fastnerf_occ_classify(grid, n, S, rays11, z, idx, cnt, raw, cws, stream)))
        return rc;
      return modes[math_mode].fwd_list(0, n, S, rays11, z, params, packed, raw, idx, cnt, flags, stream);
    }
    for (int s0 = 0; s0 < S; s0 += block) {
      const int s1 = (S - s0 > block) ? s0 + block : S;
      if ((rc = fastnerf_ert_classify(grid, cascade, n, S, s0, s1, rays11, z, s0 ? trans_ws : nullptr, eps, idx, seg, raw, cws, stream)))
        return rc;
      if ((rc = modes[math_mode].fwd_list(0, n, S, rays11, z, params, packed, raw, idx, seg, flags, stream))) return rc;
      if ((rc = fastnerf_ert_advance(n, S, s0, s1, raw, z, rays11, s0 == 0, trans_ws, seg, cnt, stream))) return rc;
    }
    return 0;
  });
}

// ---- the marched round: what the marched render and the marched step share ----------------------------------------------------
// The limits of a packed row: lists index slots with int32 and the counters are int32.  (fastnerf_step_march_ws_ints knows no K: K = 2
// asks no more of n than C >= 2 does.)
static bool march_kc_ok(int K, int C) { return K >= 2 && K < (1 << 24) && C >= 2 && C <= 512; }
static bool march_n_ok(int64_t n, int K, int C) { return n * (int64_t)C < ((int64_t)1 << 31) && n * (int64_t)K < ((int64_t)1 << 31); }

// A round's scratch, cut from one run of int32: list [n * B] | scan scratch | the segment's (count, entries) | per-ray state [2 n]
// [| transmittance [n], where the run was sized with it].  B: the most slots a round places per ray.
struct MarchWs {
  int32_t *idx, *cws, *seg, *state;
  float* trans;
};
static int64_t march_ws_ints(int64_t n, int B, bool trans) { return n * (int64_t)B + fastnerf_compact_ws_ints(n * (int64_t)B) + 2 + (trans ? 3 : 2) * n; }
static MarchWs march_ws(int32_t* p, int64_t n, int B) {
  int32_t* cws = p + n * (int64_t)B;
  int32_t* seg = cws + fastnerf_compact_ws_ints(n * (int64_t)B);
  return {p, cws, seg, seg + 2, reinterpret_cast<float*>(seg + 2 + 2 * n)};
}

// the packed rows [n, C] of one network and where the round's counters go
struct MarchRow {
  int math_mode, K, C, flags;
  int64_t n;
  const float *rays11, *params, *packed;
  float *z, *raw;
  int32_t *kidx, *counts;
  fn_stream_t stream;
};

// The round, once: place() fills the slots [s0, s1) of every row (fastnerf_occ_march or fastnerf_occ_march_jitter: the caller's
// launch), fastnerf_march_list lists the live ones (and zeroes the logits of the others), the list forward evaluates them on the packed
// z with S = C, and -- with ert, before a further round -- fastnerf_ert_advance carries the transmittance that cuts that round.
template <class Place>
static int march_round(const MarchRow& r, const MarchWs& w, int s0, int s1, bool ert, Place&& place) {
  int rc;
  if ((rc = place())) return rc;
  if ((rc = fastnerf_march_list(r.n, r.C, s0, s1, r.kidx, w.idx, w.seg, r.raw, w.cws, r.counts, (int32_t)(r.n * (int64_t)r.K), r.stream)))
    return rc;
  if ((rc = modes[r.math_mode].fwd_list(0, r.n, r.C, r.rays11, r.z, r.params, r.packed, r.raw, w.idx, w.seg, r.flags, r.stream))) return rc;
  if (ert && s1 < r.C) return fastnerf_ert_advance(r.n, r.C, s0, s1, r.raw, r.z, r.rays11, s0 == 0, w.trans, nullptr, nullptr, r.stream);
  return 0;
}

// The marched render (include/fastnerf.h, "marched render"): no sampler and no coarse pass.  Rounds of march_round, placed by
// fastnerf_occ_march, then one fastnerf_raw2outputs_fwd over [n, C].  The scratch is the stream's library-owned workspace, slot WS_MARCH.
extern "C" int fastnerf_render_rays_fwd_march(int math_mode, int64_t n, int K, int C, const float* rays11, int lindisp, int white_bkgd,
                                              const float* params, const float* packed, const fn_occ_grid* grid,
                                              const fn_occ_cascade* cascade, float eps, int block, int32_t* counts_out, float* z,
                                              int32_t* kidx, uint8_t* overflow, float* raw, float* rgb, float* disp, float* acc, float* w,
                                              float* depth, int flags, fn_stream_t stream) {
  const char* fname = "fastnerf_render_rays_fwd_march";
  if (math_mode < 0 || math_mode > 2 || n < 0 || !march_kc_ok(K, C)) {
    fn::set_error("%s: bad argument: math_mode in {0,1,2}, n >= 0, 2 <= K < 2^24, 2 <= C <= 512", fname);
    return -1;
  }
  if (block != 0 && (!(eps >= 0.f && eps < 1.f) || block < 1)) {   // block == 0: no early ray termination, one round
    fn::set_error("%s: bad argument: 0 <= eps < 1, block >= 1 (block == 0: no early ray termination)", fname);
    return -1;
  }
  if ((grid != nullptr) == (cascade != nullptr)) {
    fn::set_error("%s: bad argument: exactly one of grid / cascade", fname);
    return -1;
  }
  if (n == 0) return 0;
  if (!march_n_ok(n, K, C)) {
    fn::set_error("%s: bad argument: n * C < 2^31 (lists index slots with int32), n * K < 2^31 (the counters are int32)", fname);
    return -1;
  }
  if (!rays11 || !params || !packed || !counts_out || !z || !kidx || !overflow || !raw || !rgb || !disp || !acc || !w || !depth) {
    fn::set_error("%s: null pointer", fname);
    return -1;
  }
  if (const char* fault = cascade ? fn::occ_cascade_fault(cascade) : fn::occ_grid_fault(grid)) {   // before anything is enqueued
    fn::set_error("%s: bad argument: %s", fname, fault);
    return -1;
  }
  const int B = (block == 0 || block > C) ? C : block;
  const int64_t ints = march_ws_ints(n, B, true);
  static const fn::WsName what = {"fastnerf: no memory for the %.1f MB scratch of the marched render\n", 1e-6};
  const fn::StreamWs sw = fn::stream_ws(fn::WS_MARCH, fn::S(stream), ints, what);
  if (!sw.p) {
    fn::set_error("%s: no workspace (the stream is capturing, or there is no memory for %lld int32)", fname, (long long)ints);
    return -1;
  }
  const MarchWs ws = march_ws(reinterpret_cast<int32_t*>(sw.p), n, B);
  const MarchRow row = {math_mode, K, C, flags, n, rays11, params, packed, z, raw, kidx, counts_out, stream};
  for (int s0 = 0; s0 < C; s0 += B) {
    const int s1 = (C - s0 > B) ? s0 + B : C;
    if (int rc = march_round(row, ws, s0, s1, block != 0, [&] {
          return fastnerf_occ_march(grid, cascade, n, K, lindisp, rays11, C, s0, s1, s0 == 0, (block && s0) ? ws.trans : nullptr, eps, ws.state, z,
                                    kidx, overflow, stream);
        }))
      return rc;
  }
  return fastnerf_raw2outputs_fwd(n, C, raw, z, rays11, nullptr, white_bkgd, rgb, disp, acc, w, depth, stream);
}

extern "C" int fastnerf_render_rays_fwd(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11,
                                        int lindisp, int perturb, int det, int white_bkgd, const float* t_rand, const float* u,
                                        const float* noise0, const float* noise1, uint64_t seed0, uint64_t seed1,
                                        const float* params_c, const float* packed_c, const float* params_f,
                                        const float* packed_f, float* z0, float* raw0, float* act0, float* rgb0,
                                        float* disp0, float* acc0, float* w0, float* depth0, float* z1,
                                        float* z_samples, float* z_std, float* raw1, float* act1, float* rgb1,
                                        float* disp1, float* acc1, float* w1, float* depth1, fn_stream_t stream) {
  return fastnerf_render_rays_fwd_ex(math_mode, n, N_samples, N_importance, rays11, lindisp, perturb, det, white_bkgd, t_rand, u,
                                     noise0, noise1, seed0, seed1, params_c, packed_c, params_f, packed_f, z0, raw0, act0, rgb0,
                                     disp0, acc0, w0, depth0, z1, z_samples, z_std, raw1, act1, rgb1, disp1, acc1, w1, depth1, 0,
                                     stream);
}

// Backward of the same chain (autograd of render.py:238-299 w.r.t. the network parameters; sample positions are
// detached in the reference, so the coarse net only sees d(loss)/d(rgb0)): compositing backward -> MLP backward for the
// fine pass (into grads_f) and the coarse pass (into grads_c).  draw_ws: n * (N_samples + N_importance) * 4 floats.
// passes: bit 0 = the fine pass (N_importance > 0 only), bit 1 = the coarse pass (the only one when N_importance == 0)
// dact_ws / partial_ws hold the LAST pass's values on return -- the coarse pass's, or the fine pass's after the paired backward (below)
//
// Map gradients (fn_map_grads: every map of render.py:149-192 differentiable, as under the reference's autograd): what one pass's
// compositing backward gets beside g_rgb.  A pass without any makes exactly the fastnerf_raw2outputs_bwd call it always made; a pass
// with one goes through fastnerf_raw2outputs_bwd_full (g_rgb may then be NULL), at every site, the paired one included -- the trunk
// jobs never read draw, so pairing is untouched.
struct PassMaps {
  const float *acc, *depth, *g_disp, *g_acc, *g_depth;
  const float* g_w = nullptr;   // [n,S]: a gradient of the pass's weights themselves (fn_weight_grads: the distortion term)
  bool any() const { return g_disp || g_acc || g_depth || g_w; }
};
// pass 1 = the pass that produces the image (the only pass when N_importance == 0, where it runs on the coarse buffers), 0 = the coarse pass
static PassMaps pass_maps(const fn_map_grads* m, const fn_weight_grads* wg, int pass, const float* acc, const float* depth) {
  PassMaps q = {acc, depth, nullptr, nullptr, nullptr};
  if (m) q = pass ? PassMaps{acc, depth, m->g_disp1, m->g_acc1, m->g_depth1} : PassMaps{acc, depth, m->g_disp0, m->g_acc0, m->g_depth0};
  if (wg) q.g_w = pass ? wg->g_w1 : wg->g_w0;
  return q;
}

// One pass of a backward, in the style of RrFwd: its S samples, the forward's tensors over them, the gradients that come in, the network, and
// where its gradient goes.  act: the activations the forward saved (plain backward only); packed_fwd and counts -- where the pass's
// (live, total) goes -- the compacted backward only.
struct BwdPass {
  int S;
  const float *z, *raw, *noise, *g_rgb;
  PassMaps maps;
  const float *params, *packed_fwd, *packed_bwd, *act;
  float* grads;
  int32_t* counts;
  bool has_gradient() const { return g_rgb || maps.any(); }
  bool disp_needs_maps() const { return maps.g_disp && (!maps.acc || !maps.depth); }
};
// two == false: `coarse` is the only pass (and the one that produces the image); `fine` is then unused
struct BwdPasses { bool two; BwdPass fine, coarse; };
// what the passes of one backward share.  passes: bit 0 = the fine pass, bit 1 = the coarse pass; act_ws / live_ws: the compacted backward only
struct RrBwd {
  int math_mode, white_bkgd, passes;
  int64_t n;
  const float* rays11;
  float *draw_ws, *dact_ws, *partial_ws, *act_ws;
  int32_t* live_ws;
  fn_stream_t stream;
  int rebuild = 0;   // rr_bwd, bf16x6: 1 -- the view job rebuilds dYv and dX does not store it (train_step); 2 -- and dact_yv is poisoned first
};
static int comp_bwd(const RrBwd& c, const BwdPass& q) {
  const PassMaps& m = q.maps;
  if (!m.any()) return fastnerf_raw2outputs_bwd(c.n, q.S, q.raw, q.z, c.rays11, q.noise, c.white_bkgd, q.g_rgb, c.draw_ws, c.stream);
  return fastnerf_raw2outputs_bwd_full(c.n, q.S, q.raw, q.z, c.rays11, q.noise, c.white_bkgd, m.acc, m.depth, q.g_rgb, m.g_disp, m.g_acc, m.g_w,
                                       m.g_depth, c.draw_ws, c.stream);
}

// The ONE place that decides which buffers carry which pass, from the flat list of the entry points / the fields of fn_step_args.  With one
// pass only (N_importance == 0) the coarse buffers carry the image pass: its colour gradient is g_rgb and its map gradients are the *1
// members.  counts: 4 int32 = (live, total) of the fine pass, then of the coarse pass (the only pass writes the second pair), or NULL.
// (fine.S < coarse.S says N_importance < 0 to the checks.)
static BwdPasses bwd_passes(int N_samples, int N_importance, const float* g_rgb, const float* g_rgb0, const float* noise0, const float* noise1,
                            const float* z0, const float* raw0, const float* act0, const float* z1, const float* raw1, const float* act1,
                            const float* params_c, const float* packed_fwd_c, const float* packed_bwd_c, const float* params_f,
                            const float* packed_fwd_f, const float* packed_bwd_f, float* grads_c, float* grads_f, const float* acc0,
                            const float* depth0, const float* acc1, const float* depth1, const fn_map_grads* mg, const fn_weight_grads* wg,
                            int32_t* counts) {
  const bool two = N_importance > 0;
  return {two,
          {N_samples + N_importance, z1, raw1, noise1, g_rgb, pass_maps(mg, wg, 1, acc1, depth1), params_f, packed_fwd_f, packed_bwd_f, act1,
           grads_f, counts},
          {N_samples, z0, raw0, noise0, two ? g_rgb0 : g_rgb, pass_maps(mg, wg, two ? 0 : 1, acc0, depth0), params_c, packed_fwd_c, packed_bwd_c,
           act0, grads_c, counts ? counts + 2 : nullptr}};
}

// the checks of both backwards up to the gradients' presence; live: the compacted backward
static bool rr_bwd_checks(const RrBwd& c, const BwdPasses& p, bool live, const char* fname) {
  const BwdPass &f = p.fine, &k = p.coarse;
  if (c.math_mode < 0 || c.math_mode > 2 || c.n <= 0 || k.S < 2 || f.S < k.S) {
    fn::set_error("%s: bad argument: math_mode in {0,1,2}, n>0, N_samples>=2, N_importance>=0", fname);
    return false;
  }
  auto net = [&](const BwdPass& q) { return q.z && q.raw && q.params && q.packed_bwd && q.grads && (live ? q.packed_fwd : q.act); };
  if (!c.rays11 || !net(k) || !c.draw_ws || !c.dact_ws || !c.partial_ws || (live && (!c.act_ws || !c.live_ws))) {
    fn::set_error("%s: null pointer (coarse pass)", fname);
    return false;
  }
  if (p.two && (!f.has_gradient() || !k.has_gradient() || !net(f))) {
    fn::set_error("%s: null pointer (fine pass)", fname);
    return false;
  }
  if (!k.has_gradient()) {      // (one pass: with two, the check above has covered it)
    fn::set_error("%s: null gradient", fname);
    return false;
  }
  return true;
}

static int rr_bwd(const RrBwd& c, const BwdPasses& p) {
  const char* fname = "fastnerf_render_rays_bwd";
  const BwdPass &f = p.fine, &k = p.coarse;
  if (!rr_bwd_checks(c, p, false, fname)) return -1;
  if ((p.two && f.disp_needs_maps()) || k.disp_needs_maps()) {
    fn::set_error("%s: a disparity gradient needs the forward's acc and depth of its pass", fname);
    return -1;
  }
  int rc;
  const bool reb = c.rebuild && c.math_mode == 2;
  const SideRb rb = {1, c.rebuild == 2};
  auto run = [&](const BwdPass& q) {
    if ((rc = comp_bwd(c, q))) return rc;
    if (reb)
      return fn::x6_bwd_rebuild(c.n, q.S, c.draw_ws, q.act, q.params, q.packed_bwd, c.dact_ws, c.partial_ws, q.grads, c.stream, &rb);
    return modes[c.math_mode].bwd(0, c.n, q.S, c.draw_ws, q.act, q.params, q.packed_bwd, c.dact_ws, c.partial_ws, q.grads, c.stream);
  };
  // Both passes in this call, bf16x6: the paired backward.  The trunk dW jobs of the two passes (7 jobs of 256 x 256 each) go into ONE
  // launch behind both passes' other kernels, so the coarse pass runs on a second dact / partial set of the library's (the fine pass's must
  // survive it); draw_ws is shared as before: the trunk jobs do not read it.  Same kernels on the same data as the two passes below, in another
  // order: bit-identical gradients.  Phase-split calls, the other math modes and N_importance == 0 never come here.
  float *dact2 = nullptr, *partial2 = nullptr;
  if (p.two && c.passes == 3 && c.math_mode == 2 && fn::x6_pair_workspace(c.n * (int64_t)k.S, c.stream, &dact2, &partial2)) {
    DwDeferred d_fine, d_coarse;   // (this call's own: nothing of a call outlives it but the workspace)
    if ((rc = comp_bwd(c, f))) return rc;
    if ((rc = fn::x6_pair_pass(&d_fine, c.n, f.S, c.draw_ws, f.act, f.params, f.packed_bwd, c.dact_ws, c.partial_ws, f.grads, c.stream,
                               reb ? &rb : nullptr)))
      return rc;
    if ((rc = comp_bwd(c, k))) return rc;
    if ((rc = fn::x6_pair_pass(&d_coarse, c.n, k.S, c.draw_ws, k.act, k.params, k.packed_bwd, dact2, partial2, k.grads, c.stream,
                               reb ? &rb : nullptr)))
      return rc;
    return fn::x6_pair_finish(&d_fine, &d_coarse, c.stream);
  }
  if (p.two && (c.passes & 1) && (rc = run(f))) return rc;
  return (c.passes & 2) ? run(k) : 0;
}

extern "C" int fastnerf_render_rays_bwd_w(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11,
                                          int white_bkgd, const float* g_rgb, const float* g_rgb0, const float* noise0,
                                          const float* noise1, const float* z0, const float* raw0, const float* act0,
                                          const float* z1, const float* raw1, const float* act1, const float* params_c,
                                          const float* packed_bwd_c, const float* params_f, const float* packed_bwd_f,
                                          float* draw_ws, float* dact_ws, float* partial_ws, float* grads_c, float* grads_f,
                                          const float* acc0, const float* depth0, const float* acc1, const float* depth1,
                                          const fn_map_grads* maps, const fn_weight_grads* wg, fn_stream_t stream) {
  return rr_bwd({math_mode, white_bkgd, 3, n, rays11, draw_ws, dact_ws, partial_ws, nullptr, nullptr, stream},
                bwd_passes(N_samples, N_importance, g_rgb, g_rgb0, noise0, noise1, z0, raw0, act0, z1, raw1, act1, params_c, nullptr,
                           packed_bwd_c, params_f, nullptr, packed_bwd_f, grads_c, grads_f, acc0, depth0, acc1, depth1, maps, wg, nullptr));
}

extern "C" int fastnerf_render_rays_bwd_maps(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11,
                                             int white_bkgd, const float* g_rgb, const float* g_rgb0, const float* noise0,
                                             const float* noise1, const float* z0, const float* raw0, const float* act0,
                                             const float* z1, const float* raw1, const float* act1, const float* params_c,
                                             const float* packed_bwd_c, const float* params_f, const float* packed_bwd_f,
                                             float* draw_ws, float* dact_ws, float* partial_ws, float* grads_c, float* grads_f,
                                             const float* acc0, const float* depth0, const float* acc1, const float* depth1,
                                             const fn_map_grads* maps, fn_stream_t stream) {
  return fastnerf_render_rays_bwd_w(math_mode, n, N_samples, N_importance, rays11, white_bkgd, g_rgb, g_rgb0, noise0, noise1, z0, raw0, act0,
                                    z1, raw1, act1, params_c, packed_bwd_c, params_f, packed_bwd_f, draw_ws, dact_ws, partial_ws, grads_c,
                                    grads_f, acc0, depth0, acc1, depth1, maps, nullptr, stream);
}

extern "C" int fastnerf_render_rays_bwd(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11,
                                        int white_bkgd, const float* g_rgb, const float* g_rgb0, const float* noise0,
                                        const float* noise1, const float* z0, const float* raw0, const float* act0,
                                        const float* z1, const float* raw1, const float* act1, const float* params_c,
                                        const float* packed_bwd_c, const float* params_f, const float* packed_bwd_f,
                                        float* draw_ws, float* dact_ws, float* partial_ws, float* grads_c, float* grads_f,
                                        fn_stream_t stream) {
  return fastnerf_render_rays_bwd_maps(math_mode, n, N_samples, N_importance, rays11, white_bkgd, g_rgb, g_rgb0, noise0, noise1, z0, raw0,
                                       act0, z1, raw1, act1, params_c, packed_bwd_c, params_f, packed_bwd_f, draw_ws, dact_ws, partial_ws,
                                       grads_c, grads_f, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

// Training backward with exact zero-gradient point compaction (math_mode 1: split-bf16 kernels, 0: exact-fp32 kernels).  The forward ran WITHOUT saving
// activations (the inference kernels); per pass:  compositing backward -> list of the points with a non-zero
// d(loss)/d(raw) (fastnerf_compact_live) -> forward over that list, saving activations -> dX / dW over that list.
// The gradients equal fastnerf_render_rays_bwd's up to fp32 summation order (the dead points' terms are exact zeros).
// No host round trip: the list length stays on the device.  live_ws: 4 + n*S1 + fastnerf_compact_ws_ints(n*S1) int32;
// act_ws: fastnerf_mlp_bf16_floats(0, 3, n*S1) / fastnerf_mlp_act_floats(0, n*S1) floats; counts_out (optional): 4 int32 = live/total fine, live/total coarse
// (without it the counters stay in the first 4 int32 of live_ws).
static int rr_bwd_live(const RrBwd& c, const BwdPasses& p) {
  const char* fname = "fastnerf_render_rays_bwd_live";
  const BwdPass &f = p.fine, &k = p.coarse;
  if (!rr_bwd_checks(c, p, true, fname)) return -1;
  int32_t* idx = c.live_ws + 4;   // behind the [4] counters: list | scan scratch, sized for the longer pass
  int32_t* cws = idx + c.n * (int64_t)(p.two ? f.S : k.S);
  int rc;
  auto run = [&](const BwdPass& q) -> int {
    if (q.disp_needs_maps()) {
      fn::set_error("%s: a disparity gradient needs the forward's acc and depth of its pass", fname);
      return -1;
    }
    if ((rc = comp_bwd(c, q))) return rc;
    if ((rc = fastnerf_compact_live(c.n * (int64_t)q.S, c.draw_ws, idx, q.counts, cws, c.stream))) return rc;
    if ((rc = modes[c.math_mode].fwd_live(0, c.n, q.S, c.rays11, q.z, q.params, q.packed_fwd, c.act_ws, idx, q.counts, c.stream))) return rc;
    return modes[c.math_mode].bwd_live(0, c.n, q.S, c.draw_ws, c.act_ws, q.params, q.packed_bwd, c.dact_ws, c.partial_ws, q.grads, idx, q.counts,
                                       c.stream);
  };
  if (p.two && (c.passes & 1) && (rc = run(f))) return rc;
  return (c.passes & 2) ? run(k) : 0;
}

extern "C" int fastnerf_render_rays_bwd_live_w(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11,
                                               int white_bkgd, const float* g_rgb, const float* g_rgb0, const float* noise0,
                                               const float* noise1, const float* z0, const float* raw0, const float* z1,
                                               const float* raw1, const float* params_c, const float* packed_fwd_c,
                                               const float* packed_bwd_c, const float* params_f, const float* packed_fwd_f,
                                               const float* packed_bwd_f, float* draw_ws, float* act_ws, float* dact_ws,
                                               float* partial_ws, int32_t* live_ws, float* grads_c, float* grads_f,
                                               int32_t* counts_out, const float* acc0, const float* depth0, const float* acc1,
                                               const float* depth1, const fn_map_grads* maps, const fn_weight_grads* wg,
                                               fn_stream_t stream) {
  return rr_bwd_live({math_mode, white_bkgd, 3, n, rays11, draw_ws, dact_ws, partial_ws, act_ws, live_ws, stream},
                     bwd_passes(N_samples, N_importance, g_rgb, g_rgb0, noise0, noise1, z0, raw0, nullptr, z1, raw1, nullptr, params_c,
                                packed_fwd_c, packed_bwd_c, params_f, packed_fwd_f, packed_bwd_f, grads_c, grads_f, acc0, depth0, acc1, depth1,
                                maps, wg, counts_out ? counts_out : live_ws));
}

extern "C" int fastnerf_render_rays_bwd_live_maps(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11,
                                                  int white_bkgd, const float* g_rgb, const float* g_rgb0, const float* noise0,
                                                  const float* noise1, const float* z0, const float* raw0, const float* z1,
                                                  const float* raw1, const float* params_c, const float* packed_fwd_c,
                                                  const float* packed_bwd_c, const float* params_f, const float* packed_fwd_f,
                                                  const float* packed_bwd_f, float* draw_ws, float* act_ws, float* dact_ws,
                                                  float* partial_ws, int32_t* live_ws, float* grads_c, float* grads_f,
                                                  int32_t* counts_out, const float* acc0, const float* depth0, const float* acc1,
                                                  const float* depth1, const fn_map_grads* maps, fn_stream_t stream) {
  return fastnerf_render_rays_bwd_live_w(math_mode, n, N_samples, N_importance, rays11, white_bkgd, g_rgb, g_rgb0, noise0, noise1, z0, raw0,
                                         z1, raw1, params_c, packed_fwd_c, packed_bwd_c, params_f, packed_fwd_f, packed_bwd_f, draw_ws,
                                         act_ws, dact_ws, partial_ws, live_ws, grads_c, grads_f, counts_out, acc0, depth0, acc1, depth1,
                                         maps, nullptr, stream);
}

extern "C" int fastnerf_render_rays_bwd_live(int math_mode, int64_t n, int N_samples, int N_importance, const float* rays11, int white_bkgd,
                                             const float* g_rgb, const float* g_rgb0, const float* noise0, const float* noise1,
                                             const float* z0, const float* raw0, const float* z1, const float* raw1,
                                             const float* params_c, const float* packed_fwd_c, const float* packed_bwd_c,
                                             const float* params_f, const float* packed_fwd_f, const float* packed_bwd_f,
                                             float* draw_ws, float* act_ws, float* dact_ws, float* partial_ws, int32_t* live_ws,
                                             float* grads_c, float* grads_f, int32_t* counts_out, fn_stream_t stream) {
  return fastnerf_render_rays_bwd_live_maps(math_mode, n, N_samples, N_importance, rays11, white_bkgd, g_rgb, g_rgb0, noise0, noise1, z0, raw0,
                                            z1, raw1, params_c, packed_fwd_c, packed_bwd_c, params_f, packed_fwd_f, packed_bwd_f, draw_ws,
                                            act_ws, dact_ws, partial_ws, live_ws, grads_c, grads_f, counts_out, nullptr, nullptr, nullptr,
                                            nullptr, nullptr, stream);
}


// ---------------------------------------------------------------------------------------------------------------------
// One optimisation step of the reference's loop (run_nerf.py:479-508: render -> img2mse (fine + coarse) -> loss.backward() ->
// optimizer.step(); the leaf-error table of :505-506 is fed inside the loss launch) enqueued by ONE call -- or by one call
// per phase when the caller interleaves its gradient all-reduce (data parallel: the fine net's gradient is final after
// FN_STEP_BWD_FINE and travels while FN_STEP_BWD_COARSE runs).  Exactly the launches the entry points above make, in the same
// order, on the caller's stream: results are bit-identical to calling them one by one.  (One exception to "the same order", not to the
// results: a call with both backward phases in bf16x6 runs the paired backward of rr_bwd -- one trunk dW launch for both passes.)
// The two steps, fastnerf_train_step and fastnerf_train_step_march, share the stages below.
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int64_t fastnerf_step_args_size(void) { return (int64_t)sizeof(fn_step_args); }

extern "C" int64_t fastnerf_step_aux_size(void) { return (int64_t)sizeof(fn_step_aux); }

extern "C" int64_t fastnerf_step_bkgd_size(void) { return (int64_t)sizeof(fn_step_bkgd); }

extern "C" int64_t fastnerf_step_dist_size(void) { return (int64_t)sizeof(fn_step_dist); }

extern "C" int64_t fastnerf_step_expo_size(void) { return (int64_t)sizeof(fn_step_expo); }

// the refusals of a step with the exposure table (ex != NULL), before anything of the step is launched; the struct is read in a forward phase only
static bool step_expo_ok(const fn_step_args* a, const fn_step_expo* ex, bool two, int phases, const char* fname) {
  if (ex->n_img < 1 || !(ex->lambda >= 0.0f) || !(ex->lambda < __builtin_huge_valf()) || a->n >= ((int64_t)1 << 31)) {
    fn::set_error("%s: bad argument: n_img >= 1, lambda >= 0 and finite, n < 2^31", fname);
    return false;
  }
  if ((phases & FN_STEP_FORWARD) &&
      (!ex->img || !ex->ab || !ex->e1 || (two && !ex->e0) || !ex->ws || !ex->d_ab || !ex->counts || !ex->loss_reg)) {
    fn::set_error("%s: null member of fn_step_expo (img, ab, e1, ws, d_ab, counts, loss_reg; e0 with two passes)", fname);
    return false;
  }
  return true;
}

// the refusals of a step with the distortion term (dist != NULL, lambda_dist != 0), before anything of the step is launched.  w1 / w0: the
// weights of the image pass / of the coarse pass of two (NULL with one pass), as the step's forward leaves them
static bool step_dist_ok(const fn_step_dist* d, bool two, int phases, const float* w1, const float* w0, const char* fname) {
  if (!(d->lambda_dist > 0.0f) || !(d->lambda_dist < __builtin_huge_valf())) {
    fn::set_error("%s: bad argument: lambda_dist >= 0 and finite", fname);
    return false;
  }
  const bool fwd = (phases & FN_STEP_FORWARD) != 0;
  const bool any = (phases & (FN_STEP_FORWARD | FN_STEP_BWD_FINE | FN_STEP_BWD_COARSE)) != 0;
  if ((any && (!d->g_w1 || (two && !d->g_w0))) || (fwd && (!d->ell1 || (two && !d->ell0) || !d->loss2d))) {
    fn::set_error("%s: null member of fn_step_dist (g_w1, ell1, loss2d; g_w0, ell0 with two passes)", fname);
    return false;
  }
  if (fwd && (!w1 || (two && !w0))) {
    fn::set_error("%s: the distortion term needs the weights of its pass (w0, w1)", fname);
    return false;
  }
  return true;
}

// the refusals of a step with per-ray background colours (bk != NULL), before anything else of the step is looked at
static bool step_bkgd_ok(const fn_step_args* a, const fn_step_bkgd* bk, bool two, int phases, const char* fname) {
  if (a->white_bkgd) {
    fn::set_error("%s: white_bkgd != 0 cannot be combined with per-ray background colours (bkgd = ones is white)", fname);
    return false;
  }
  const bool fwd = (phases & FN_STEP_FORWARD) != 0;
  const bool maps = (phases & (FN_STEP_FORWARD | FN_STEP_BWD_FINE | FN_STEP_BWD_COARSE)) != 0;
  if ((fwd && (!bk->bkgd_used || !bk->target_ws)) || (maps && (!bk->g_acc1 || (two && !bk->g_acc0)))) {
    fn::set_error("%s: null member of fn_step_bkgd (bkgd_used, target_ws, g_acc1, g_acc0 with two passes)", fname);
    return false;
  }
  if (fwd && ((bk->bkgd != nullptr) == (bk->seed != 0))) {
    fn::set_error("%s: exactly one of fn_step_bkgd.bkgd and seed != 0", fname);
    return false;
  }
  return true;
}

// the refusals of a step whose first forward runs over a list: it is a compacted step, without sigma noise; `what` / `who`: the caller's words
static bool step_list_ok(const fn_step_args* a, const char* fname, const char* what, const char* who) {
  if (!a->live) {
    fn::set_error("%s: %s (live != 0): the plain backward has no list", fname, what);
    return false;
  }
  if (a->noise0 || a->noise1) {
    fn::set_error("%s: %s cannot be combined with sigma noise (it is added before the relu)", fname, who);
    return false;
  }
  return true;
}

// a step through a cascade: it stands where a->occ would, so a->occ is NULL, and every level is usable -- before anything is enqueued
static bool step_cascade_ok(const fn_step_args* a, const fn_occ_cascade* cascade, const char* fname) {
  if (a->occ) {
    fn::set_error("%s: bad argument: a cascade needs args->occ == NULL (one of the two)", fname);
    return false;
  }
  if (const char* fault = fn::occ_cascade_fault(cascade)) {
    fn::set_error("%s: bad argument: %s", fname, fault);
    return false;
  }
  return true;
}

// the rays of the batch -> rays11; with FN_STEP_TIGHTEN near / far of every ray are then clamped to what the grid's bits, as they are
// now, leave occupied (cascade != NULL: the cascade's, a->occ being NULL then).  rays11 persists to the backward.
static int step_pack_rays(const fn_step_args* a, const fn_occ_cascade* cascade, fn_stream_t stream) {
  if (int rc = fastnerf_pack_rays(a->n, a->rays_o, a->rays_d, a->near_plane, a->far_plane, a->ndc, a->H, a->W, a->focal, a->rays11, stream))
    return rc;
  return (a->fwd_flags & FN_STEP_TIGHTEN) ? fastnerf_occ_ray_bounds(cascade ? nullptr : a->occ, cascade, a->n, a->rays11, 1, nullptr, nullptr, stream) : 0;
}

// One pass as the loss launches see it: its maps, weights and depths [n, S], and the colour gradient they leave for its backward.
struct LossPass { float* rgb; const float *acc, *depth, *w, *z; int S; float* g_rgb; };
// the pass in the *0 buffers of fn_step_args: the coarse pass of two, the image pass of one, the marched row
static LossPass loss_pass0(const fn_step_args* a, int S, float* g_rgb) { return {a->rgb0, a->acc0, a->depth0, a->w0, a->z0, S, g_rgb}; }

// The loss launches of a forward phase, behind its render, of both steps: blend -> exposure -> mse_leafmax -> depth / opacity terms -> overflow mask ->
// what the exposure sends back to the table (and takes out of the colour gradient) -> what the blend sends back to acc -> distortion.  p1: the image
// pass; p0: the coarse pass of two, {} with one.  aux / bk / dist / ex: NULL = the term is off.  mask: NULL, or the marched step's overflow flags (never
// with aux).  A new term is a few lines here; its checks stay with the callers', before any launch.
static int step_losses(const fn_step_args* a, const LossPass& p1, const LossPass& p0, const fn_step_aux* aux, const fn_step_bkgd* bk,
                       const fn_step_dist* dist, const fn_step_expo* ex, const uint8_t* mask, fn_stream_t stream) {
  const bool two = p0.S > 0;
  int rc;
  // (bk: white_bkgd is 0 -- the forward left the bare maps; the colours go behind them and behind the target here)
  if (bk &&
      (rc = fastnerf_bkgd_blend(a->n, bk->bkgd, bk->seed, bk->alpha, p1.acc, p0.acc, p1.rgb, p0.rgb, a->target, bk->target_ws, bk->bkgd_used, stream)))
    return rc;
  // (ex: the colour loss and the leaf table see the re-exposed maps e; rgb stays the scene's colour)
  float* e0 = (ex && two) ? ex->e0 : nullptr;
  if (ex && (rc = fastnerf_expo_apply(a->n, ex->n_img, ex->img, ex->ab, p1.rgb, p0.rgb, ex->e1, e0, stream))) return rc;
  if ((rc = fastnerf_mse_leafmax(a->n, ex ? ex->e1 : p1.rgb, ex ? e0 : p0.rgb, bk ? bk->target_ws : a->target, a->grad_scale, p1.g_rgb, p0.g_rgb,
                                 a->loss2, a->leaf_tag, a->max_leaves, a->table, stream)))
    return rc;
  if (aux && (rc = fastnerf_aux_loss(a->n, p1.depth, p1.acc, p0.depth, p0.acc, aux->depth_target, aux->depth_weight, aux->acc_target, aux->acc_weight,
                                     aux->lambda_depth, aux->lambda_acc, a->grad_scale, aux->g_depth1, aux->g_acc1, two ? aux->g_depth0 : nullptr,
                                     two ? aux->g_acc0 : nullptr, aux->loss4, stream)))
    return rc;
  // a truncated row has lost what lies behind the cut: its colour error does not train the field (loss2 stays the mean over all rays)
  if (mask && (rc = fastnerf_march_mask(a->n, mask, p1.g_rgb, stream))) return rc;
  // behind the mask (a masked ray has G = 0: nothing for the table) and in front of every reader of the colour gradient, which it rescales in place
  if (ex && (rc = fastnerf_expo_grad(a->n, ex->n_img, ex->img, ex->ab, ex->lambda, a->grad_scale, ex->e1, e0, p1.g_rgb, p0.g_rgb, ex->ws, ex->d_ab,
                                     ex->counts, ex->loss_reg, stream)))
    return rc;
  // what the blend sends back to acc, on top of the opacity term's rows when that term is on (behind the mask: an overflowed ray's g_acc is +-0)
  if (bk) {
    const bool add = aux && aux->acc_target;
    if ((rc = fastnerf_bkgd_grad(a->n, bk->bkgd_used, p1.g_rgb, p0.g_rgb, add ? aux->g_acc1 : nullptr, (add && two) ? aux->g_acc0 : nullptr,
                                 bk->g_acc1, two ? bk->g_acc0 : nullptr, stream)))
      return rc;
  }
  if (!dist) return 0;      // per pass l and coef * dl/dw (skip = mask: a truncated row's weights are an artefact too), then the batch means
  const float coef = (float)((double)a->grad_scale * (double)dist->lambda_dist / (double)a->n);
  if ((rc = fastnerf_distortion(a->n, p1.S, p1.w, p1.z, a->rays11, a->lindisp, mask, coef, nullptr, dist->ell1, dist->g_w1, stream))) return rc;
  if (two && (rc = fastnerf_distortion(a->n, p0.S, p0.w, p0.z, a->rays11, a->lindisp, mask, coef, nullptr, dist->ell0, dist->g_w0, stream))) return rc;
  return fastnerf_distortion_mean(a->n, dist->ell1, two ? dist->ell0 : nullptr, dist->loss2d, stream);
}

static bool step_update_ok(const fn_step_args* a, const char* fname) {
  if (a->adam_m && a->adam_v && a->adam_t >= 1) return true;
  fn::set_error("%s: update phase needs adam_m, adam_v and adam_t >= 1", fname);
  return false;
}

// the update phase over the networks [first, first + count) of the flat buffer: ONE Adam launch over their parameters, then each one's re-pack
static int step_update(const fn_step_args* a, int first, int count, fn_stream_t stream) {
  const int64_t off = first * a->net_floats;
  if (int rc = fastnerf_adam_step(count * a->net_floats, a->params + off, a->grads + off, a->adam_m + off, a->adam_v + off, a->lr, a->beta1,
                                  a->beta2, a->eps, a->adam_t, stream))
    return rc;
  for (int k = first; k < first + count; k++)
    if (int rc = modes[a->math_mode].pack(0, a->params + k * a->net_floats, k ? a->packed_fwd_f : a->packed_fwd_c,
                                          k ? a->packed_bwd_f : a->packed_bwd_c, stream))
      return rc;
  return 0;
}

// aux: NULL, or the depth / opacity terms (a term is on when its target is set); bk: NULL, or the per-ray background colours; dist: NULL,
// or the distortion term (on when lambda_dist != 0); ex: NULL, or the exposure table; cascade: NULL, or the occupancy cascade that takes
// the place of a->occ at each of its sites (step_cascade_ok: a->occ is NULL then)
static int train_step(const fn_step_args* a, const fn_step_aux* aux, const fn_step_bkgd* bk, const fn_step_dist* dist, const fn_step_expo* ex,
                      const fn_occ_cascade* cascade, int phases, fn_stream_t stream) {
  if (dist && dist->lambda_dist == 0.0f) dist = nullptr;
  const char* fname = cascade ? "fastnerf_train_step_cascade"
                      : ex    ? "fastnerf_train_step_expo"
                      : dist  ? "fastnerf_train_step_dist"
                      : bk    ? "fastnerf_train_step_bkgd"
                              : "fastnerf_train_step";
  if (aux && !aux->depth_target && !aux->acc_target) aux = nullptr;
  if (!a || a->math_mode < 0 || a->math_mode > 2 || a->n <= 0 || a->N_samples < 2 || a->N_importance < 0) {
    fn::set_error("%s: bad argument: args != NULL, math_mode in {0,1,2}, n>0, N_samples>=2, N_importance>=0", fname);
    return -1;
  }
  if (cascade && !step_cascade_ok(a, cascade, fname)) return -1;
  const bool two = a->N_importance > 0;
  if (bk && !step_bkgd_ok(a, bk, two, phases, fname)) return -1;
  if (dist && !step_dist_ok(dist, two, phases, two ? a->w1 : a->w0, two ? a->w0 : nullptr, fname)) return -1;
  if (ex && !step_expo_ok(a, ex, two, phases, fname)) return -1;
  if (bk && aux && aux->acc_target && (phases & FN_STEP_FORWARD) && (!aux->g_acc1 || (two && !aux->g_acc0))) {
    fn::set_error("%s: null gradient buffer of the opacity term (its rows are added to the background's)", fname);
    return -1;
  }
  if (!a->params || !a->grads || !a->packed_fwd_c || !a->packed_bwd_c || (two && (!a->packed_fwd_f || !a->packed_bwd_f)) ||
      a->net_floats <= 0) {
    fn::set_error("%s: null network buffer", fname);
    return -1;
  }
  if (a->occ || cascade) {
    // the grid removes samples from the FIRST forward of a compacted step; the plain backward has no list to run over, and sigma
    // noise is added before the relu: a sample with zero sigma is not dead then
    if (!step_list_ok(a, fname, "an occupancy grid needs the compacted step", "an occupancy grid")) return -1;
    if (!a->live_ws) {
      fn::set_error("%s: an occupancy grid needs live_ws", fname);
      return -1;
    }
  } else if (a->fwd_flags & FN_STEP_TIGHTEN) {
    fn::set_error("%s: FN_STEP_TIGHTEN needs an occupancy grid (occ != NULL)", fname);
    return -1;
  }
  const int passes = ((phases & FN_STEP_BWD_FINE) ? 1 : 0) | ((phases & FN_STEP_BWD_COARSE) ? 2 : 0);
  // (every refusal before the first launch: a forward phase in the same call would have run by the time the backward looks)
  if (passes && aux && ((aux->depth_target && (!aux->g_depth1 || (two && !aux->g_depth0))) ||
                        (aux->acc_target && (!aux->g_acc1 || (two && !aux->g_acc0))))) {
    fn::set_error("%s: null gradient buffer of a term whose target is set", bk ? fname : "fastnerf_train_step_aux");
    return -1;
  }
  if ((phases & FN_STEP_UPDATE) && !step_update_ok(a, fname)) return -1;
  const int fwd_flags = a->fwd_flags & ~FN_STEP_TIGHTEN;   // the step's own bit does not travel on to the forward
  // The rebuilding view job (dw_pair.h SideRb) with dX's store of dYv off: the backward passes of a step in bf16x6 on the plain backward.  dact_ws
  // is the step's own scratch and the view job of the same pass is the only reader of dact_yv in it -- fastnerf_ray_grad, which reads it too, is
  // a call of its own behind a backward that stored (render.py), never part of a step.  FASTNERF_SIDE_REBUILD=0: the reading route.
  const int rebuild = (passes && a->math_mode == 2 && !a->live) ? fn::side_rebuild_mode() : 0;
  const float* params_c = a->params;
  const float* params_f = two ? a->params + a->net_floats : nullptr;
  int rc;
  if (phases & FN_STEP_FORWARD) {
    if (!a->rays_o || !a->rays_d || !a->target || !a->rays11 || !a->g_rgb || (two && !a->g_rgb0) || !a->loss2) {
      fn::set_error("%s: null batch / output buffer", fname);
      return -1;
    }
    if ((rc = step_pack_rays(a, cascade, stream))) return rc;
    const bool save = !a->live;
    if (cascade) {      // the grid's call below, argument for argument: rr_fwd_occ is the one body of both
      if ((rc = fastnerf_render_rays_fwd_occ_cascade(a->math_mode, a->n, a->N_samples, a->N_importance, a->rays11, a->lindisp,
                                                     (a->perturb || a->t_rand) ? 1 : 0, a->perturb ? 0 : 1, a->white_bkgd, a->t_rand, a->u,
                                                     a->seed0, a->seed1, params_c, a->packed_fwd_c, params_f, a->packed_fwd_f, cascade,
                                                     a->live_ws + 4, a->occ_counts ? a->occ_counts : a->live_ws, a->z0, a->raw0, a->rgb0,
                                                     a->disp0, a->acc0, a->w0, a->depth0, a->z1, a->z_samples, a->z_std, a->raw1, a->rgb1,
                                                     a->disp1, a->acc1, a->w1, a->depth1, fwd_flags, stream)))
        return rc;
    } else if (a->occ) {
      // live_ws: [4] counters of the backward | list | scan scratch -- the forward's list and scratch are dead before the backward
      // writes its own; without occ_counts the forward's counters land in the backward's (which overwrites them)
      if ((rc = fastnerf_render_rays_fwd_occ(a->math_mode, a->n, a->N_samples, a->N_importance, a->rays11, a->lindisp,
                                             (a->perturb || a->t_rand) ? 1 : 0, a->perturb ? 0 : 1, a->white_bkgd, a->t_rand, a->u,
                                             a->seed0, a->seed1, params_c, a->packed_fwd_c, params_f, a->packed_fwd_f, a->occ,
                                             a->live_ws + 4, a->occ_counts ? a->occ_counts : a->live_ws, a->z0, a->raw0, a->rgb0,
                                             a->disp0, a->acc0, a->w0, a->depth0, a->z1, a->z_samples, a->z_std, a->raw1, a->rgb1,
                                             a->disp1, a->acc1, a->w1, a->depth1, fwd_flags, stream)))
        return rc;
    } else if ((rc = fastnerf_render_rays_fwd_ex(a->math_mode, a->n, a->N_samples, a->N_importance, a->rays11, a->lindisp,
                                          (a->perturb || a->t_rand) ? 1 : 0, a->perturb ? 0 : 1, a->white_bkgd, a->t_rand, a->u,
                                          a->noise0, a->noise1, a->seed0, a->seed1, params_c, a->packed_fwd_c, params_f,
                                          a->packed_fwd_f, a->z0, a->raw0, save ? a->act0 : nullptr, a->rgb0, a->disp0, a->acc0,
                                          a->w0, a->depth0, a->z1, a->z_samples, a->z_std, a->raw1, save ? a->act1 : nullptr,
                                          a->rgb1, a->disp1, a->acc1, a->w1, a->depth1, save ? 0 : fwd_flags, stream)))
      return rc;
    const LossPass p0 = loss_pass0(a, a->N_samples, two ? a->g_rgb0 : a->g_rgb);
    const LossPass p1 = {a->rgb1, a->acc1, a->depth1, a->w1, a->z1, a->N_samples + a->N_importance, a->g_rgb};
    if ((rc = step_losses(a, two ? p1 : p0, two ? p0 : LossPass{}, aux, bk, dist, ex, nullptr, stream))) return rc;
  }
  if (passes) {
    fn_map_grads mg = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (aux) {
      // (the *0 members are read with two passes only: bwd_passes)
      if (aux->depth_target) { mg.g_depth1 = aux->g_depth1; mg.g_depth0 = aux->g_depth0; }
      if (aux->acc_target) { mg.g_acc1 = aux->g_acc1; mg.g_acc0 = aux->g_acc0; }
    }
    if (bk) { mg.g_acc1 = bk->g_acc1; mg.g_acc0 = bk->g_acc0; }      // (they hold the opacity term's rows too: fastnerf_bkgd_grad)
    const fn_weight_grads wg = {dist ? dist->g_w1 : nullptr, dist ? dist->g_w0 : nullptr};
    const RrBwd c = {a->math_mode, a->white_bkgd, passes, a->n, a->rays11, a->draw_ws, a->dact_ws, a->partial_ws, a->act_ws, a->live_ws, stream,
                     rebuild};
    const BwdPasses p = bwd_passes(a->N_samples, a->N_importance, a->g_rgb, a->g_rgb0, a->noise0, a->noise1, a->z0, a->raw0, a->act0, a->z1,
                                   a->raw1, a->act1, params_c, a->packed_fwd_c, a->packed_bwd_c, params_f, a->packed_fwd_f, a->packed_bwd_f,
                                   a->grads, two ? a->grads + a->net_floats : nullptr, a->acc0, a->depth0, a->acc1, a->depth1,
                                   (aux || bk) ? &mg : nullptr, dist ? &wg : nullptr, a->counts ? a->counts : a->live_ws);
    if ((rc = a->live ? rr_bwd_live(c, p) : rr_bwd(c, p))) return rc;
  }
  if (phases & FN_STEP_UPDATE) return step_update(a, 0, two ? 2 : 1, stream);
  return 0;
}

extern "C" int fastnerf_train_step(const fn_step_args* a, int phases, fn_stream_t stream) {
  return train_step(a, nullptr, nullptr, nullptr, nullptr, nullptr, phases, stream);
}

extern "C" int fastnerf_train_step_aux(const fn_step_args* a, const fn_step_aux* aux, int phases, fn_stream_t stream) {
  return train_step(a, aux, nullptr, nullptr, nullptr, nullptr, phases, stream);
}

extern "C" int fastnerf_train_step_bkgd(const fn_step_args* a, const fn_step_aux* aux, const fn_step_bkgd* bk, int phases,
                                        fn_stream_t stream) {
  return train_step(a, aux, bk, nullptr, nullptr, nullptr, phases, stream);
}

extern "C" int fastnerf_train_step_dist(const fn_step_args* a, const fn_step_aux* aux, const fn_step_bkgd* bk, const fn_step_dist* dist,
                                        int phases, fn_stream_t stream) {
  return train_step(a, aux, bk, dist, nullptr, nullptr, phases, stream);
}

extern "C" int fastnerf_train_step_expo(const fn_step_args* a, const fn_step_aux* aux, const fn_step_bkgd* bk, const fn_step_dist* dist,
                                        const fn_step_expo* ex, int phases, fn_stream_t stream) {
  return train_step(a, aux, bk, dist, ex, nullptr, phases, stream);
}

extern "C" int fastnerf_train_step_cascade(const fn_step_args* a, const fn_step_aux* aux, const fn_step_bkgd* bk, const fn_step_dist* dist,
                                           const fn_step_expo* ex, const fn_occ_cascade* cascade, int phases, fn_stream_t stream) {
  return train_step(a, aux, bk, dist, ex, cascade, phases, stream);
}

// The marched step (include/fastnerf.h, "marched training"): one network on the packed rows of a jittered lattice.  The row is [n, C] in
// the *0 buffers of fn_step_args; the forward is ONE march_round placed by fastnerf_occ_march_jitter, on the caller's list_ws; the backward
// is rr_bwd_live over the row as a single pass of C samples -- closing and padding slots hold zero logits, whose d(loss)/d(raw) is exactly
// zero, so they never enter its list.  Every check comes before the first launch.
extern "C" int64_t fastnerf_step_march_size(void) { return (int64_t)sizeof(fn_step_march); }

extern "C" int64_t fastnerf_step_march_ws_ints(int64_t n, int C) {
  if (n <= 0 || !march_kc_ok(2, C) || !march_n_ok(n, 2, C)) return -1;
  return march_ws_ints(n, C, false);
}

static int train_step_march(const fn_step_args* a, const fn_step_march* mx, const fn_step_bkgd* bk, const fn_step_dist* dist,
                            const fn_step_expo* ex, const fn_occ_cascade* cascade, int phases, fn_stream_t stream) {
  if (dist && dist->lambda_dist == 0.0f) dist = nullptr;
  const char* fname = cascade ? "fastnerf_train_step_march_cascade"
                      : ex   ? "fastnerf_train_step_march_expo"
                      : dist ? "fastnerf_train_step_march_dist"
                      : bk   ? "fastnerf_train_step_march_bkgd"
                             : "fastnerf_train_step_march";
  if (!a || !mx || a->math_mode < 0 || a->math_mode > 2 || a->n <= 0 || mx->which < 0 || mx->which > 1) {
    fn::set_error("%s: bad argument: args and march != NULL, math_mode in {0,1,2}, n > 0, which in {0,1}", fname);
    return -1;
  }
  if (cascade && !step_cascade_ok(a, cascade, fname)) return -1;
  if (bk && !step_bkgd_ok(a, bk, false, phases, fname)) return -1;
  if (dist && !step_dist_ok(dist, false, phases & ~FN_STEP_BWD_FINE, a->w0, nullptr, fname)) return -1;
  if (ex && !step_expo_ok(a, ex, false, phases, fname)) return -1;
  const int K = mx->K, C = mx->C;
  const int64_t n = a->n;
  if (!march_kc_ok(K, C) || !march_n_ok(n, K, C)) {
    fn::set_error("%s: bad argument: 2 <= K < 2^24, 2 <= C <= 512, n * C < 2^31, n * K < 2^31", fname);
    return -1;
  }
  if (!a->occ && !cascade) {
    fn::set_error("%s: the march walks an occupancy grid (occ != NULL)", fname);
    return -1;
  }
  if (!step_list_ok(a, fname, "the marched step is a compacted step", "the march")) return -1;
  if (const char* fault = cascade ? nullptr : fn::occ_grid_fault(a->occ)) {
    fn::set_error("%s: bad argument: %s", fname, fault);
    return -1;
  }
  float* pf = mx->which ? a->packed_fwd_f : a->packed_fwd_c;
  float* pb = mx->which ? a->packed_bwd_f : a->packed_bwd_c;
  if (!a->params || !a->grads || !pf || !pb || a->net_floats <= 0 || !a->rays11 || !a->z0 || !a->raw0 || !a->g_rgb || !mx->kidx ||
      !mx->overflow || !mx->list_ws || !mx->counts) {
    fn::set_error("%s: null network, row or march buffer", fname);
    return -1;
  }
  const int64_t off = mx->which ? a->net_floats : 0;
  const float* params = a->params + off;
  const bool bwd = (phases & FN_STEP_BWD_COARSE) != 0;
  if ((phases & FN_STEP_FORWARD) && (!a->rays_o || !a->rays_d || !a->target || !a->loss2 || !a->rgb0 || !a->disp0 || !a->acc0 || !a->w0 ||
                                     !a->depth0)) {
    fn::set_error("%s: null batch / output buffer", fname);
    return -1;
  }
  if (bwd && (!a->draw_ws || !a->act_ws || !a->dact_ws || !a->partial_ws || !a->live_ws)) {
    fn::set_error("%s: null scratch of the compacted backward", fname);
    return -1;
  }
  if ((phases & FN_STEP_UPDATE) && !step_update_ok(a, fname)) return -1;
  int rc;
  if (phases & FN_STEP_FORWARD) {
    const MarchWs ws = march_ws(mx->list_ws, n, C);      // (fastnerf_step_march_ws_ints: no transmittance)
    const MarchRow row = {a->math_mode, K, C, a->fwd_flags & ~FN_STEP_TIGHTEN, n, a->rays11, params, pf, a->z0, a->raw0, mx->kidx, mx->counts, stream};
    if ((rc = step_pack_rays(a, cascade, stream))) return rc;
    if ((rc = march_round(row, ws, 0, C, false, [&] {
           return fastnerf_occ_march_jitter(cascade ? nullptr : a->occ, cascade, n, K, a->lindisp, a->rays11, C, 0, C, 1, nullptr, 0.f, mx->u, mx->seed, ws.state,
                                            a->z0, mx->kidx, mx->overflow, stream);
         })))
      return rc;
    if ((rc = fastnerf_raw2outputs_fwd(n, C, a->raw0, a->z0, a->rays11, nullptr, a->white_bkgd, a->rgb0, a->disp0, a->acc0, a->w0, a->depth0,
                                       stream)))
      return rc;
    if ((rc = step_losses(a, loss_pass0(a, C, a->g_rgb), {}, nullptr, bk, dist, ex, mx->overflow, stream))) return rc;
  }
  if (bwd) {
    // the single pass, built directly (one pass: both members of BwdPasses name it); its counters are the coarse pair, as after a one-pass
    // fastnerf_train_step
    PassMaps maps = bk ? PassMaps{a->acc0, a->depth0, nullptr, bk->g_acc1, nullptr} : PassMaps{};
    if (dist) maps.g_w = dist->g_w1;
    const BwdPass pass = {C, a->z0, a->raw0, nullptr, a->g_rgb, maps,
                          params, pf, pb, nullptr,
                          a->grads + off, (a->counts ? a->counts : a->live_ws) + 2};
    if ((rc = rr_bwd_live({a->math_mode, a->white_bkgd, 2, n, a->rays11, a->draw_ws, a->dact_ws, a->partial_ws, a->act_ws, a->live_ws, stream},
                          {false, pass, pass})))
      return rc;
  }
  if (phases & FN_STEP_UPDATE) return step_update(a, mx->which, 1, stream);
  return 0;
}

extern "C" int fastnerf_train_step_march(const fn_step_args* a, const fn_step_march* mx, int phases, fn_stream_t stream) {
  return train_step_march(a, mx, nullptr, nullptr, nullptr, nullptr, phases, stream);
}

extern "C" int fastnerf_train_step_march_bkgd(const fn_step_args* a, const fn_step_march* mx, const fn_step_bkgd* bk, int phases,
                                              fn_stream_t stream) {
  return train_step_march(a, mx, bk, nullptr, nullptr, nullptr, phases, stream);
}

extern "C" int fastnerf_train_step_march_dist(const fn_step_args* a, const fn_step_march* mx, const fn_step_bkgd* bk, const fn_step_dist* dist,
                                              int phases, fn_stream_t stream) {
  return train_step_march(a, mx, bk, dist, nullptr, nullptr, phases, stream);
}

extern "C" int fastnerf_train_step_march_expo(const fn_step_args* a, const fn_step_march* mx, const fn_step_bkgd* bk, const fn_step_dist* dist,
                                              const fn_step_expo* ex, int phases, fn_stream_t stream) {
  return train_step_march(a, mx, bk, dist, ex, nullptr, phases, stream);
}

extern "C" int fastnerf_train_step_march_cascade(const fn_step_args* a, const fn_step_march* mx, const fn_step_bkgd* bk, const fn_step_dist* dist,
                                                 const fn_step_expo* ex, const fn_occ_cascade* cascade, int phases, fn_stream_t stream) {
  return train_step_march(a, mx, bk, dist, ex, cascade, phases, stream);
}
