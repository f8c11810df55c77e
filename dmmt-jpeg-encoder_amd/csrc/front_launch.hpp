// front_launch.hpp -- the grid of a front kernel (kernels.hip: k_front,
// k_front_surf; front_ycc.hip: k_front_ycc): host code shared by their launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <algorithm>

namespace dmmt {

static inline int clampi(long long v, int lo, int hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }

// The resident workgroups of one front-kernel instantiation: one workgroup per
// resident slot, each looping over tiles and prefetching the next.  A launcher
// keeps one as a function static, computed once (thread-safe initialisation).
struct FrontCfg {
    int resident, n_cus;
    bool per_cu_env;
};
template <typename K>
static FrontCfg front_cfg(K kernel) {
    int per_cu = 0, dev = 0, cus = 0;
    bool env = false;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess || per_cu < 1) per_cu = 2;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
        cus = 256;
    if (const char* e = getenv("DMMT_FRONT_PER_CU")) {  // tuning knob (both lane modes)
        per_cu = atoi(e) > 0 ? atoi(e) : per_cu;
        env = true;
    }
    return FrontCfg{per_cu * cus, cus, env};
}
// per_cu_cap: fewer resident workgroups per CU (a context of several lanes)
static inline dim3 front_grid(const FrontCfg& cfg, long long ntiles, int n_frames, int per_cu_cap) {
    const int res = per_cu_cap > 0 && !cfg.per_cu_env ? std::min(cfg.resident, per_cu_cap * cfg.n_cus) : cfg.resident;
    return dim3(clampi(ntiles, 1, res / n_frames > 0 ? res / n_frames : 1), n_frames);
}

}  // namespace dmmt
