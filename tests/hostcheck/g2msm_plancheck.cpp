// tests/hostcheck/g2msm_plancheck.cpp — TEST-ONLY driver for a plain g++ build (no GPU, no library) of csrc/g2msm_plan.h: the lines of the
// grid of g2msm_plan_grid.h on stdout (one per plan of one blob, then one per group of a batched call), a line on stderr and exit status
// 1 per violated invariant.  Built and run by tests/test_g2msm_plan_host.py and tests/test_g2msm_batch_plan_host.py.
#include "g2msm_plan_grid.h"

int main() {
    const int failures = g2grid::run(stdout);
    return failures ? 1 : 0;
}
