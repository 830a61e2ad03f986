// register_fit_check.cpp -- csrc/rtr_register_fit.h as a stand-alone host program (tests/test_cpp_register.py builds it with
// g++ -ffp-contract=off -fno-fast-math, once plain and once with -fsanitize=address,undefined).  Reads records from the
// file named by argv[1], one per line: the mode (0 point-to-point, 1 point-to-plane), the 32 moments and the 12 doubles
// of a pose, every double as the 16 hex digits of its bits.  Prints per record: degenerate, the 12 doubles of the step,
// the 12 of step o pose and the rms residual, in the same form.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rtr_register_fit.h"

static double from_bits(uint64_t b) {
    double d;
    memcpy(&d, &b, sizeof d);
    return d;
}
static uint64_t to_bits(double d) {
    uint64_t b;
    memcpy(&b, &d, sizeof b);
    return b;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    int mode, records = 0;
    while (fscanf(f, "%d", &mode) == 1) {
        double mom[RTR_REGISTER_MOMENTS], pose[12], step[12], next[12];
        uint64_t b;
        for (int i = 0; i < RTR_REGISTER_MOMENTS; ++i) {
            if (fscanf(f, "%" SCNx64, &b) != 1) return 3;
            mom[i] = from_bits(b);
        }
        for (int i = 0; i < 12; ++i) {
            if (fscanf(f, "%" SCNx64, &b) != 1) return 3;
            pose[i] = from_bits(b);
        }
        const bool deg = mode ? rtr::register_fit_plane(mom, step) : rtr::register_fit_point(mom, step);
        rtr::register_compose(step, pose, next);
        const double rms = rtr::register_rms(mom[mode ? rtr::kRegPlaneResidual : rtr::kRegPointResidual], mom[0]);
        printf("%d", deg ? 1 : 0);
        for (int i = 0; i < 12; ++i) printf(" %016" PRIx64, to_bits(step[i]));
        for (int i = 0; i < 12; ++i) printf(" %016" PRIx64, to_bits(next[i]));
        printf(" %016" PRIx64 "\n", to_bits(rms));
        ++records;
    }
    fclose(f);
    return records ? 0 : 4;
}
