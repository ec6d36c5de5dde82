// Which farthest-point-sampling kernel afm_fps launches for a sample of n points and m samples to draw, and with what launch shape.
// Pure host arithmetic (no HIP header, no allocation, no launch; valid C and C++): tests/test_fps_plan_host.py compiles it on its own and
// walks every n.  csrc/pointops.hip instantiates exactly the (form, ppt) pairs this rule can return.
#pragma once

typedef enum {
    FPS_UNSUPPORTED = 0,     // n > 16384: more than 32 points per thread on 512 threads
    FPS_PRUNED,              // fps_pruned_kernel<ppt, 1024>: Morton-sorted cells, exact pruning of the per-round scan
    FPS_PLAIN_LDS,           // fps_kernel<ppt, ., true>: every point scanned every round, the winner's coordinates read from an LDS copy
    FPS_PLAIN_GLOBAL         // fps_kernel<32, 512, false>: the sample does not fit in LDS, the winner's coordinates come from global memory
} FpsForm;

typedef struct {
    FpsForm form;
    int ppt;                 // points per thread the kernel is instantiated for: 2 / 4 / 8 (pruned), 1 / 2 / 4 / 8 / 16 / 32 (plain)
    int threads;             // per workgroup (one workgroup per sample)
    int lds_bytes;           // dynamic LDS of the launch, <= FPS_LDS_LIMIT
} FpsPlan;

enum { FPS_LDS_LIMIT = 150 * 1024, FPS_MAX_POINTS = 16384 };

static inline FpsPlan fps_plan(int n, int m) {
    FpsPlan p = {FPS_UNSUPPORTED, 0, 0, 0};
    if (n < 1 || n > FPS_MAX_POINTS) return p;
    if (n >= 1536 && n <= 8192 && m >= 32) {
        // pruned form: 1024 threads own np2 / 1024 Morton-consecutive points each.  Below 32 samples the sort does not pay, below 1536 points
        // the plain kernel's round is already short.  LDS holds the sort arrays (2 np2 words) first, then the [3n] copy of the sample.
        int np2 = 2048;
        while (np2 < n) np2 <<= 1;
        p.form = FPS_PRUNED; p.ppt = np2 / 1024; p.threads = 1024;
        p.lds_bytes = 4 * (3 * n > 2 * np2 ? 3 * n : 2 * np2);
        return p;
    }
    // plain form.  Threads per workgroup: a round is a dependent chain (per-thread scan -> wave arg-max -> LDS hop -> barrier -> broadcast) on ONE
    // compute unit per sample.  Its VALU work (n points x 8 instructions: ~1100 issue cycles of the ~2100-cycle round at n = 8192) is
    // the same for every split, the reductions are not: 0.94 / 0.96 / 0.91 us per round with 1024 / 512 / 256 threads
    // (profiles/r02_points_probe.txt) - so 32 points per thread on as few waves as hold them.  Results do not depend on the split.
    const int T = (((n + 31) / 32 + 63) / 64) * 64;  // 64 ... 512 for 1 <= n <= FPS_MAX_POINTS
    const int ppt = (n + T - 1) / T;                 // <= 32
    p.ppt = ppt <= 1 ? 1 : ppt <= 2 ? 2 : ppt <= 4 ? 4 : ppt <= 8 ? 8 : ppt <= 16 ? 16 : 32;
    p.threads = T;
    p.form = 12 * n <= FPS_LDS_LIMIT ? FPS_PLAIN_LDS : FPS_PLAIN_GLOBAL;       // n > 12800 implies ppt > 16: the global form exists for 32 only
    p.lds_bytes = p.form == FPS_PLAIN_LDS ? 12 * n : 0;
    return p;
}
