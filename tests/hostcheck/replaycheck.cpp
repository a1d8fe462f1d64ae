// Host build of the UNCHECKED mixed addition of csrc/curve.h (xyzz_madd<.., false>, the form k_msm_accumulate's loop uses) beside the
// checked one, with -DKZG_BOUND_CHECK: every lazy-reduction bound aborts, also on the values a sum carries after it met P == +-Q.
// Test infrastructure (tests/test_accumulate_replay_host.py), not a CPU fallback.
#include <cstdint>
#include "field29.h"
#include "curve.h"

using namespace kzg;

extern "C" {

// pts_wire: n affine wire points (16 u32 each, identity = zeros), neg[i] = 1: subtract.  Adds them in order, once with the unchecked
// and once with the checked addition (identity points skipped, as the kernels do).
//   *tainted        fe_is_zero_mod(ZZ) of the unchecked sum (0 when it is still the identity flag)
//   limbs_unchecked 36 limbs X | Y | ZZ | ZZZ of the unchecked sum, limbs_checked the same of the checked one, *inf_* their flags
//   wire_checked    the checked sum as 32 u32 wire words X || Y || ZZ || ZZZ
void kzg_rc_chain(const uint32_t* pts_wire, const uint32_t* neg, uint32_t n, uint32_t* tainted, int32_t* limbs_unchecked, uint32_t* inf_unchecked,
                  int32_t* limbs_checked, uint32_t* inf_checked, uint32_t* wire_checked) {
    Xyzz u, c;
    xyzz_set_inf(u);
    xyzz_set_inf(c);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t dev[16];
        uint32_t any = 0;
        for (int j = 0; j < 16; ++j) any |= pts_wire[16 * i + j];
        if (any == 0) continue;
        affine_wire_to_device(dev, pts_wire + 16 * i);
        Affine p;
        fe_unpack(p.x, dev);
        fe_unpack(p.y, dev + 8);
        xyzz_madd<true, false>(u, p, neg[i]);
        xyzz_madd<true, true>(c, p, neg[i]);
    }
    *tainted = (!u.inf && fe_is_zero_mod(u.zz)) ? 1u : 0u;
    const Fq* cu[4] = {&u.x, &u.y, &u.zz, &u.zzz};
    const Fq* cc[4] = {&c.x, &c.y, &c.zz, &c.zzz};
    for (int q = 0; q < 4; ++q)
        for (int j = 0; j < NL; ++j) { limbs_unchecked[q * NL + j] = cu[q]->l[j]; limbs_checked[q * NL + j] = cc[q]->l[j]; }
    *inf_unchecked = u.inf ? 1u : 0u;
    *inf_checked = c.inf ? 1u : 0u;
    xyzz_to_wire(wire_checked, c);
}

}  // extern "C"
