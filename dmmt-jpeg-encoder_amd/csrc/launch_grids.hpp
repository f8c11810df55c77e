// launch_grids.hpp -- gridDim.x of the kernels that run a capped grid and loop:
// the front kernels (front_launch.hpp) and k_hist (kernels.hip: launch_hist).
// Plain integer arithmetic with no HIP dependency: tests/native/launch_grid_check.cpp
// compiles this header for the host and checks it against a table
// (tests/test_launch_grids.py), and tests/tools/loop_cases.py mirrors it.
#pragma once

namespace dmmt {

static inline int clampi(long long v, int lo, int hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }

// Workgroups per frame of a front kernel: one per tile, at most the frame's share
// of the resident slots, at least 1.  resident: the instantiation's workgroups the
// device holds at once (per CU x n_cus); per_cu_cap > 0: at most that many per CU
// (a context of several lanes) -- unless per_cu_env, the DMMT_FRONT_PER_CU tuning
// knob, already chose the per-CU count.
static inline int front_grid_x(int resident, int n_cus, bool per_cu_env, long long ntiles, int n_frames,
                               int per_cu_cap) {
    const int capped = per_cu_cap * n_cus;
    const int res = per_cu_cap > 0 && !per_cu_env ? (resident < capped ? resident : capped) : resident;
    return clampi(ntiles, 1, res / n_frames > 0 ? res / n_frames : 1);
}

// Workgroups per frame of k_hist: one per 256 blocks of the bpf in a frame, at most
// the frame's share of wg_cap workgroups per launch, at least 1.
static inline int hist_grid_x(long long bpf, int n_frames, int wg_cap) {
    const int per_frame = wg_cap / n_frames > 0 ? wg_cap / n_frames : 1;
    return clampi((bpf + 255) / 256, 1, per_frame);
}

}  // namespace dmmt
