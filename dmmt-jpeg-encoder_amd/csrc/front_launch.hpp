// front_launch.hpp -- the grid and the launch of a front kernel (kernels.hip:
// k_front, k_front_surf; front_ycc.hip: k_front_ycc; front_ycc_sub.hip: k_front_ycc_sub;
// front_gray.hip: k_front_gray;
// each with a narrow twin, *_n): host code shared by their launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <type_traits>

#include "jpeg_common.hpp"
#include "launch_grids.hpp"

namespace dmmt {

// The resident workgroups of one front-kernel instantiation: one workgroup per
// resident slot, each looping over tiles and prefetching the next.
struct FrontCfg {
    int resident, n_cus;
    bool per_cu_env;
};
// max_per_cu > 0: at most so many per CU, whatever fits
template <typename K>
static FrontCfg front_cfg(K kernel, int max_per_cu) {
    int per_cu = 0, dev = 0, cus = 0;
    bool env = false;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess || per_cu < 1) per_cu = 2;
    if (max_per_cu > 0 && per_cu > max_per_cu) per_cu = max_per_cu;
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
    return dim3(front_grid_x(cfg.resident, cfg.n_cus, cfg.per_cu_env, ntiles, n_frames, per_cu_cap), n_frames);
}

// One launch of the instantiation Wide, or of its narrow twin Narrow (nullptr: it
// has none) when the call stores narrow blocks (coef_lo set): the twin takes the
// wide kernel's arguments, then coef_lo and coef_hi.  A tile is 32 / g.hr MCUs.
// Each kernel's FrontCfg is a function static, computed once (thread-safe
// initialisation).  MAX_PER_CU: the kernel's resident workgroups per CU are capped
// there (0: as many as fit).
template <auto Kernel, int MAX_PER_CU = 0, typename... Args>
static void front_launch_one(const Geom& g, int n_frames, int per_cu_cap, hipStream_t st, Args... args) {
    static const FrontCfg cfg = front_cfg(Kernel, MAX_PER_CU);
    const int tm = 32 / g.hr;
    const long long ntiles = (long long)((g.mcux + tm - 1) / tm) * g.mcuy;
    hipLaunchKernelGGL(Kernel, front_grid(cfg, ntiles, n_frames, per_cu_cap), dim3(256), 0, st, args...);
}
template <auto Wide, auto Narrow, int MAX_PER_CU = 0, typename... Args>
static void front_launch(const Geom& g, int n_frames, int per_cu_cap, hipStream_t st, int16_t* coef_lo, int8_t* coef_hi,
                         Args... args) {
    if constexpr (!std::is_null_pointer_v<decltype(Narrow)>) {
        if (coef_lo) return front_launch_one<Narrow, MAX_PER_CU>(g, n_frames, per_cu_cap, st, args..., coef_lo, coef_hi);
    }
    front_launch_one<Wide, MAX_PER_CU>(g, n_frames, per_cu_cap, st, args...);
}

// f(HR, VR) with the chroma sampling of g as two std::integral_constants: 4:4:4
// (1, 1), 4:2:2 (2, 1) or 4:2:0 (2, 2) -- the template arguments of a front kernel
template <typename F>
static void front_with_sampling(const Geom& g, F&& f) {
    using One = std::integral_constant<int, 1>;
    using Two = std::integral_constant<int, 2>;
    if (g.hr == 1)
        f(One{}, One{});
    else if (g.vr == 1)
        f(Two{}, One{});
    else
        f(Two{}, Two{});
}

}  // namespace dmmt
