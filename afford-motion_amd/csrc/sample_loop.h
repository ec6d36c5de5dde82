// Host-side pieces shared by the two native sampling-loop drivers (cmdm.hip: sample_loop_impl, perceiver.hip: cdm_sample_loop_impl):
// the arguments every loop takes, the sub-batch partition, the expanded schedule, the step noise and the events of a loop call.
// Plain structs and inline functions; nothing here allocates, and nothing launches beyond what the drivers launched before it existed.
#pragma once
#include "common.h"

// elementwise.hip
__attribute__((visibility("hidden"))) int afm_ddpm_expand_rows(const int64_t* tmap, const float* c1, const float* c2, const float* sigma, int32_t n_steps,
                                                               int32_t B, int64_t* t_all, float* c1_all, float* c2_all, float* s_all, void* stream);
__attribute__((visibility("hidden"))) int afm_ddim_expand_rows(const int64_t* tmap, const afm_ddim_rows* rows, int32_t n_steps, int32_t B, int64_t* t_all,
                                                               float4* rec_all, float* s_all, void* stream);
__attribute__((visibility("hidden"))) int afm_randn_steps(float*, int32_t, int64_t, uint64_t, int64_t, int32_t, int32_t, void*);      // [nsteps][B][per_sample]
namespace afm_loop { struct Update; }
// checks and enqueues one sampling update over B samples (AFM_E_BADARG: a NULL tensor or row, x0_u without scale or known without mask or
// the reverse, a middle branch x0_a without both scales and x0_u, a noise term without noise unless `philox`, xpad with ldpad < cols, `dpm`
// without DDIM-layout rows or with a noise term, x0_prev without `dpm`, x0_keep without `dpm` or `ddim` with `grad`, grad without gk or
// the reverse; B == 0: nothing to do)
__attribute__((visibility("hidden"))) int afm_sampling_update(const afm_loop::Update& p, int32_t B, void* stream);

// guidance.hip: afm_contact_guidance on the samples [start, start + count) of the description's batch (x, frame_mask, t, grad, energy
// already point at sample `start`; the workspace: afm_contact_guide_workspace_bytes(g, count, L) - the public size function of the
// description's form, absolute columns or h3d)
__attribute__((visibility("hidden"))) int64_t afm_contact_guide_workspace_bytes(const afm_contact_guide* g, int32_t count, int32_t L);
__attribute__((visibility("hidden"))) int afm_contact_guidance_sub(const afm_contact_guide* g, int32_t start, const float* x, const uint8_t* frame_mask,
                                                                   const int64_t* t, float* grad, float* energy, int32_t count, int32_t L, int32_t D,
                                                                   void* workspace, int64_t workspace_bytes, void* stream);

__attribute__((visibility("hidden"))) int afm_contact_guide_check(const afm_contact_guide* g, int32_t L, int32_t D);

// guidance.hip: the sum of the contact and the joint-target guidance (afm_motion_guide; either term may be missing) - its checks, the
// workspace of `count` samples of a checked sum, and afm_motion_guidance on the samples [start, start + count), computing the terms named
__attribute__((visibility("hidden"))) int afm_motion_guide_check(const afm_motion_guide* g, int32_t L, int32_t D);
__attribute__((visibility("hidden"))) int64_t afm_motion_guide_workspace_bytes(const afm_motion_guide* g, int32_t count, int32_t L, int32_t D);
__attribute__((visibility("hidden"))) int afm_motion_guidance_sub(const afm_motion_guide* g, bool run_contact, bool run_targets, int32_t start, const float* x,
                                                                  const uint8_t* frame_mask, const int64_t* t, float* grad, float* energy_contact,
                                                                  float* energy_targets, int32_t count, int32_t L, int32_t D, void* workspace,
                                                                  int64_t workspace_bytes, void* stream);

// guidance.hip: the sum with the scene clearance (afm_scene_guide, taken apart: `terms` NULL or a sum with a term set, `clear` NULL or the
// clearance; at least one) - its checks, the workspace of `count` samples of a checked sum (clear == NULL: afm_motion_guide_workspace_bytes
// exactly), and afm_scene_guidance on the samples [start, start + count), computing the terms named (clear == NULL: afm_motion_guidance_sub)
__attribute__((visibility("hidden"))) int afm_scene_guide_check(const afm_motion_guide* terms, const afm_scene_clearance* clear, int32_t L, int32_t D);
__attribute__((visibility("hidden"))) int64_t afm_scene_guide_workspace_bytes(const afm_motion_guide* terms, const afm_scene_clearance* clear, int32_t count,
                                                                              int32_t L, int32_t D);
__attribute__((visibility("hidden"))) int afm_scene_guidance_sub(const afm_motion_guide* terms, const afm_scene_clearance* clear, bool run_contact,
                                                                 bool run_targets, bool run_clear, int32_t start, const float* x, const uint8_t* frame_mask,
                                                                 const int64_t* t, float* grad, float* energy_contact, float* energy_targets,
                                                                 float* energy_clear, int32_t count, int32_t L, int32_t D, void* workspace,
                                                                 int64_t workspace_bytes, void* stream);

// guidance.hip: the sum with the foot grounding (afm_ground_guide, taken apart: `terms` and `clear` as above, `feet` NULL or the grounding;
// at least one of the three) - its checks, the workspace of `count` samples of a checked sum and afm_ground_guidance on the samples
// [start, start + count), computing the terms named.  feet == NULL: the three functions above, exactly.
__attribute__((visibility("hidden"))) int afm_ground_guide_check(const afm_motion_guide* terms, const afm_scene_clearance* clear,
                                                                 const afm_foot_grounding* feet, int32_t L, int32_t D);
__attribute__((visibility("hidden"))) int64_t afm_ground_guide_workspace_bytes(const afm_motion_guide* terms, const afm_scene_clearance* clear,
                                                                               const afm_foot_grounding* feet, int32_t count, int32_t L, int32_t D);
__attribute__((visibility("hidden"))) int afm_ground_guidance_sub(const afm_motion_guide* terms, const afm_scene_clearance* clear,
                                                                  const afm_foot_grounding* feet, bool run_contact, bool run_targets, bool run_clear,
                                                                  bool run_feet, int32_t start, const float* x, const uint8_t* frame_mask,
                                                                  const int64_t* t, float* grad, float* energy_contact, float* energy_targets,
                                                                  float* energy_clear, float* energy_feet, int32_t count, int32_t L, int32_t D,
                                                                  void* workspace, int64_t workspace_bytes, void* stream);

// guidance.hip: the guidance of stitched long motions (afm_long_guide) - its checks, the workspace of `count` long motions of a checked
// description, and afm_long_guidance on the long motions [start, start + count) (x, t, grad point at window start * S)
__attribute__((visibility("hidden"))) int afm_long_guide_check(const afm_long_guide* g, int32_t L, int32_t D);
__attribute__((visibility("hidden"))) int64_t afm_long_guide_workspace_bytes(const afm_long_guide* g, int32_t count, int32_t L, int32_t D);
__attribute__((visibility("hidden"))) int afm_long_guidance_sub(const afm_long_guide* g, bool run_contact, bool run_targets, int32_t start, const float* x,
                                                                const int64_t* t, float* grad, float* energy_contact, float* energy_targets,
                                                                int32_t count, int32_t L, int32_t D, void* workspace, int64_t workspace_bytes,
                                                                void* stream);

// guidance.hip: the long guidance with the scene clearance next to (or without) its terms (afm_long_scene_guide, taken apart: `clear` NULL
// or the clearance; g->terms may name neither term when it is set) - its checks, the workspace of `count` long motions of a checked
// description (clear == NULL: afm_long_guide_workspace_bytes exactly), and afm_long_scene_guidance on the long motions [start, start + count)
__attribute__((visibility("hidden"))) int afm_long_scene_guide_check(const afm_long_guide* g, const afm_scene_clearance* clear, int32_t L, int32_t D);
__attribute__((visibility("hidden"))) int64_t afm_long_scene_guide_workspace_bytes(const afm_long_guide* g, const afm_scene_clearance* clear, int32_t count,
                                                                                   int32_t L, int32_t D);
__attribute__((visibility("hidden"))) int afm_long_scene_guidance_sub(const afm_long_guide* g, const afm_scene_clearance* clear, bool run_contact,
                                                                      bool run_targets, bool run_clear, int32_t start, const float* x, const int64_t* t,
                                                                      float* grad, float* energy_contact, float* energy_targets, float* energy_clear,
                                                                      int32_t count, int32_t L, int32_t D, void* workspace, int64_t workspace_bytes,
                                                                      void* stream);

namespace afm_loop {

// ---- the sampling update x_t -> x_next of one launch, [B][per_sample] floats: every DDPM, DDIM and guided update outside the fused GEMM /
// CDM output epilogues is this one description (elementwise.hip: sampling_update_kernel).
struct Update {
    const float* x0;                // pred_xstart (the conditioned branch's when guided)
    const float *x0_u, *scale;      // guided: the unconditioned branch's pred_xstart and scale [B]; both NULL: unguided
    const float *x0_a, *scale2;     // two-scale guided (cfg_combine2): the middle branch's pred_xstart (only the first condition kept) and the
                                    //   second condition's scale [B], `scale` being the first's; both NULL: one scale.  Need x0_u and scale.
    const float* known;             // imputation [B][per_sample]: x0 (guided: the combination) := mask ? known : x0, before the clamp;
    const uint8_t* mask;            //   nonzero = known; both NULL: none
    const float* xt;
    float* xn;                      // x_next; may alias xt (the loops update in place)
    const float* noise;             // NULL with a noise term: drawn in the kernel from (seed, sample0 + b, step) if `philox`, else rejected
    const float *c1, *c2, *sg;      // DDPM rows [B]; sg is also the DDIM noise coefficient (NULL there: no noise term, noise never read)
    const float *ra, *rb, *rc, *rd; // DDIM rows [B] (`ddim` set), or
    const float4* rec;              //   the same as {a, b, c, d} records [B].  With `dpm`: the 2M rows {a, b, c, unused} (rd may be NULL)
    float* xpad;                    // x_next also as rows of `cols` values at row stride ldpad (NULL: none)
    int64_t ldpad, per_sample, sample0;
    uint64_t seed;
    int cols, clip, ddim, philox, step;
    int dpm;                        // DPM-Solver++(2M) update (dpm_update of common.h) on the DDIM-layout rows; `ddim` set too, no noise term
    const float* x0_prev;           // `dpm`: the previous step's final x0 [B][per_sample]; NULL: the two-term form (never read then)
    float* x0_keep;                 // `dpm`: the final x0 (after combine, select and clamp) is also stored here; NULL: not kept.  May alias
                                    //   x0_prev (one thread reads then writes an element).  Also taken with `ddim` and `grad`: the shifted x0
    const float *grad, *gk;         // cond_fn guidance: grad [B][per_sample] = grad log p(y | x_t), gk [B] its coefficient (DDPM: the
                                    //   posterior variance, mean += gk * grad; DDIM / 2M: (1 - abar) / sqrt(abar), x0 += gk * grad after the
                                    //   clamp - the shifted x0 is what x0_keep stores); both NULL: none, grad is never read
    // stitched windows (afm_stitch): sample b is window b % st_S of long motion b / st_S, per_sample == st_L * st_D.  Between the combine
    // and the select, an element of the last st_ov frames of a window with a later neighbour, or of the first st_ov frames of one with an
    // earlier neighbour, becomes stitch_blend (common.h) of its own combined x0 and the neighbour sample's - read from the x0 buffers at
    // +- st_ov * st_D and combined with the NEIGHBOUR's scales.  Only the x0 buffers are read across samples and only the
    // element's own x_next / xpad / x0_keep are written, so the in-place update stays race-free (x0_keep must not alias an x0 buffer).
    // st_w: the weight row [2][st_ov], wl then wr.  st_S <= 1 or st_ov == 0: no blend (the unstitched kernel).  DDIM without a noise
    // term or 2M only; with grad the shift follows the clamp as in the unstitched kernel.
    int st_S, st_ov, st_L, st_D;
    const float* st_w;
    bool stitched() const { return st_S > 1 && st_ov > 0; }
};

inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// steps of Philox noise drawn per launch of a native loop (workspace: NOISE_STEPS x count x per_sample floats per sub-batch): one launch per
// NOISE_STEPS steps instead of one per step (a launch is ~5 us of a small-batch step)
constexpr int NOISE_STEPS = 16;

// what every loop entry point takes besides its model's tensors, in the order of the signatures (`ddim` == NULL: the DDPM rows c1 / c2 / sigma)
struct LoopArgs {
    const float* step_noise;
    const int64_t* tmap;
    const float *c1, *c2, *sigma;
    const afm_ddim_rows* ddim;
    int n_steps, first_step;
    uint64_t seed;
    int64_t sample_index0;
    int B;
    void *sched_scratch, *workspace;
    int64_t workspace_bytes;
    int n_streams;
    void* const* streams;
    void* stream;
    bool dpm = false;               // the 2M loop: `ddim` holds its rows as {a, b, c, d = c (unused), sigma = NULL}; no noise, no seed

    bool ok() const {
        const bool rows_ok = ddim ? (ddim->a && ddim->b && ddim->c && ddim->d) : (c1 && c2 && sigma);
        return tmap && rows_ok && n_steps > 0 && sched_scratch && workspace && n_streams >= 0 && (n_streams <= 1 || streams);
    }
    bool noise_term() const { return !ddim || ddim->sigma; }      // eta = 0 DDIM rows: no noise is generated or read
    // the library-private update selectors of the loop's own copy of a weight pack (never taken from a caller)
    uint32_t loop_flags(uint32_t flags) const {
        flags &= ~(AFM_PRIV_DDIM | AFM_PRIV_NO_NOISE);
        return ddim ? flags | AFM_PRIV_DDIM | (noise_term() ? 0 : AFM_PRIV_NO_NOISE) : flags;
    }
};

// ---- the sub-batches of a loop call: sample range [start, start + count) on `stream`
struct SubRange { int start, count; hipStream_t stream; };

inline void sub_range(int B, int n, int s, int* start, int* count) {
    const int base = B / n, extra = B % n;
    *count = base + (s < extra ? 1 : 0);
    *start = s * base + (s < extra ? s : extra);
}

// sub-batches of a batch of B on `n_streams` streams: the one rule of the loops and of their workspace-size functions
inline int sub_count(int B, int n_streams, int cap) {
    const int n = n_streams > 1 ? (n_streams < B ? n_streams : (B > 0 ? B : 1)) : 1;
    return n < cap ? n : cap;
}

// ---- the expanded schedule: per step j (timestep index n_steps - 1 - j of the slice's rows) and sample, in `sched_scratch`.
// DDPM (layout of afm_cmdm_sched_scratch_bytes): t int64 | c1 | c2 | sigma float, [n_steps][B] each.
// DDIM (layout of afm_ddim_sched_scratch_bytes): t int64 | {a, b, c, d} float4 records | s float (not written for eta = 0 rows).
struct StepRows {
    const int64_t* t;
    const float *c1, *c2, *sigma;
    const float4* rec;              // DDIM only (NULL in a DDPM loop)
};

struct Schedule {
    int B = 0;
    int64_t* t = nullptr;
    float *c1 = nullptr, *c2 = nullptr, *sigma = nullptr;
    float4* rec = nullptr;

    // lays the scratch out and enqueues the expansion on the caller's stream
    int expand(const LoopArgs& a) {
        char* sp = (char*)a.sched_scratch;
        const int64_t nb = (int64_t)a.n_steps * a.B;
        B = a.B;
        t = (int64_t*)sp; sp += align256(nb * 8);
        if (a.ddim) {
            rec = (float4*)sp; sp += align256(nb * 16);
            sigma = (float*)sp;
            return afm_ddim_expand_rows(a.tmap, a.ddim, a.n_steps, B, t, rec, sigma, a.stream);
        }
        c1 = (float*)sp; sp += align256(nb * 4);
        c2 = (float*)sp; sp += align256(nb * 4);
        sigma = (float*)sp;
        return afm_ddpm_expand_rows(a.tmap, a.c1, a.c2, a.sigma, a.n_steps, B, t, c1, c2, sigma, a.stream);
    }

    // the rows of step j from sample `start` on.  In a DDIM loop c1 == c2 == the float4 records: afm_ddpm_args has no field of that type,
    // and the AFM_UPD_DDIM epilogues (common.h) read their {a, b, c, d} through c1.  This is the only place that convention is produced;
    // host code that consumes the records takes `rec`.
    StepRows at(int j, int start) const {
        const int64_t e = (int64_t)j * B + start;
        if (rec) return StepRows{t + e, (const float*)(rec + e), (const float*)(rec + e), sigma + e, rec + e};
        return StepRows{t + e, c1 + e, c2 + e, sigma + e, nullptr};
    }
};

// ---- the step noise: (sub-batch r with its NOISE_STEPS-step workspace slot, step j; `per` values per sample) -> *out, the noise the update
// reads.  With `draw_on`, a loop that draws its own noise enqueues the next NOISE_STEPS steps' on *draw_on when j opens a block.  `unread`:
// any valid device pointer, handed out where the update never reads noise (AFM_UPD_NO_NOISE).
inline int step_noise(const LoopArgs& a, int64_t per, const SubRange& r, float* slot, int j, const float* unread, const hipStream_t* draw_on,
                      const float** out) {
    *out = unread;
    if (!a.noise_term()) return 0;
    if (a.step_noise) { *out = a.step_noise + ((int64_t)j * a.B + r.start) * per; return 0; }
    *out = slot + (int64_t)(j % NOISE_STEPS) * r.count * per;
    if (!draw_on || j % NOISE_STEPS != 0) return 0;
    return afm_randn_steps(slot, r.count, per, a.seed, a.sample_index0 + r.start, a.first_step + j,
                           a.n_steps - j < NOISE_STEPS ? a.n_steps - j : NOISE_STEPS, *draw_on);
}

// the update launch of a loop step from its stored pred_xstart: in place on x, the step's rows, noise only where the rows have a noise term
inline Update loop_update(const LoopArgs& a, const StepRows& rows, const float* x0, float* x, const float* noise, int64_t per_sample, int clip) {
    Update u = {};
    u.x0 = x0; u.xt = x; u.xn = x; u.per_sample = per_sample; u.clip = clip ? 1 : 0;
    if (rows.rec) { u.ddim = 1; u.rec = rows.rec; }
    else { u.c1 = rows.c1; u.c2 = rows.c2; }
    if (a.noise_term()) { u.sg = rows.sigma; u.noise = noise; }
    u.dpm = a.dpm ? 1 : 0;
    return u;
}

// the update arguments of (sub-batch r, step j): in place on the sub-batch's x
inline afm_ddpm_args ddpm_args(const LoopArgs& a, const StepRows& rows, const float* noise, float* xs, const SubRange& r, int j) {
    afm_ddpm_args dd = {};
    dd.noise = noise;
    dd.x_next = xs;                 // in place: each element is read then written by the same lane
    dd.c1 = rows.c1; dd.c2 = rows.c2; dd.sigma = rows.sigma;
    dd.seed = a.seed; dd.sample_index0 = a.sample_index0 + r.start; dd.step = a.first_step + j;
    return dd;
}

// ---- the events of one loop call: everything make() created is destroyed when the holder leaves scope, on every return path
struct Events {
    static constexpr int CAP = 96;  // fork + 2 per sub-batch + 2 * AFM_MAX_LAYERS of the paired schedule + one join event per sub-batch
    hipEvent_t ev[CAP];
    int n = 0;
    Events() = default;
    Events(const Events&) = delete;
    ~Events() { for (int i = 0; i < n; ++i) (void)hipEventDestroy(ev[i]); }
    int make(hipEvent_t* out) {
        if (n >= CAP) return AFM_E_UNSUPPORTED;
        if (hipEventCreateWithFlags(out, hipEventDisableTiming) != hipSuccess) return (int)hipGetLastError();
        ev[n++] = *out;
        return 0;
    }
};

// fork: the sub-batch streams start behind everything already queued on s0 (inputs, schedule rows).  SB: a struct with SubRange's `stream`.
template <class SB>
inline int fork_streams(Events& ev, hipStream_t s0, const SB* sb, int n, hipEvent_t* fork) {
    const int rc = ev.make(fork);
    if (rc != 0) return rc;
    (void)hipEventRecord(*fork, s0);
    for (int s = 0; s < n; ++s) (void)hipStreamWaitEvent(sb[s].stream, *fork, 0);
    return 0;
}

// join: s0 continues only after every sub-batch stream has finished its loop
template <class SB>
inline void join_streams(Events& ev, hipStream_t s0, const SB* sb, int n) {
    for (int s = 0; s < n; ++s) {
        hipEvent_t done;
        if (ev.make(&done) != 0) continue;
        (void)hipEventRecord(done, sb[s].stream);
        (void)hipStreamWaitEvent(s0, done, 0);
    }
}

}  // namespace afm_loop
