// Host-only C entry points around pika-zoo_amd/csrc/pz_dispatch.hpp for tests/test_dispatch.py: the instantiation the
// choice names, rendered as the demangled kernel name (tests/kernel_matrix.py's form), and the choice's image.
#include <stdio.h>

#include "pz_dispatch.hpp"

static const char* b(bool v) { return v ? "true" : "false"; }

static void render(const pz::StepKernel& s, char* out, int cap)
{
    if (s.family == pz::kStepPairKernel)
        snprintf(out, cap, "step_pair_kernel<%s, %s, %s, %s>", b(s.ai1), b(s.ai2), b(s.packed), b(s.mode == pz::kRandom));
    else if (s.family == pz::kRolloutPairKernel)
        snprintf(out, cap, "rollout_pair_kernel<%s, %s, %d, %s, %s, %s>", b(s.ai1), b(s.ai2), s.mode, b(s.packed),
                 b(s.obs16), b(s.plain));
    else
        snprintf(out, cap, "step_kernel<%s, %s, %d, %s, %d, %s, %s, %s>", b(s.ai1), b(s.ai2), s.mode, b(s.sparse), s.scout,
                 b(s.packed), b(s.obs16), b(s.plain));
}

extern "C" {

// the product's choice (no family left out)
void pz_test_choose(int mode, int k, int64_t n, const pz_config* cfg, int stats, int power_hit, char* out, int cap)
{
    render(pz::choose_step_kernel(mode, k, n, *cfg, stats != 0, power_hit != 0), out, cap);
}

// instantiation i of the product's image (if i < the count); returns the count
int pz_test_image(int i, char* out, int cap)
{
    static constexpr pz::StepKernelSet kImage = pz::step_kernel_image();
    if (i < kImage.count) render(kImage.at[i], out, cap);
    return kImage.count;
}

}  // extern "C"
