// CPU check of the capped grids (csrc/launch_grids.hpp, the launchers' own header
// compiled for the host): reads one query per line from stdin and prints
// gridDim.x, one per line.
//   f RESIDENT N_CUS PER_CU_ENV NTILES N_FRAMES PER_CU_CAP   -> front_grid_x
//   h BPF N_FRAMES WG_CAP                                     -> hist_grid_x
// tests/test_launch_grids.py feeds it a hand-computed table and a seeded sweep.
#include <stdio.h>

#include "../../dmmt-jpeg-encoder_amd/csrc/launch_grids.hpp"

int main() {
    char kind;
    int n = 0;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'f') {
            int resident, n_cus, env, n_frames, cap;
            long long ntiles;
            if (scanf("%d %d %d %lld %d %d", &resident, &n_cus, &env, &ntiles, &n_frames, &cap) != 6) return 2;
            printf("%d\n", dmmt::front_grid_x(resident, n_cus, env != 0, ntiles, n_frames, cap));
        } else if (kind == 'h') {
            long long bpf;
            int n_frames, cap;
            if (scanf("%lld %d %d", &bpf, &n_frames, &cap) != 3) return 2;
            printf("%d\n", dmmt::hist_grid_x(bpf, n_frames, cap));
        } else {
            return 2;
        }
        ++n;
    }
    fprintf(stderr, "ok: %d queries\n", n);
    return 0;
}
