// tests/hostcheck/proof_plancheck.cpp — TEST-ONLY driver for a plain g++ build (no GPU, no library) of csrc/proof_plan.h: prints the plan of every
// case of the fixed grid (proof_grid.h) in the format of tests/golden/proof_plans.txt and checks, on every plan, what the kernels of poly.hip and
// proof_enqueue rely on whatever the policy decides.  Built and run by tests/test_proof_plan_host.py and, under ASan + UBSan, by
// tests/test_sanitizers_host.py.  Exit status 1 and a line on stderr per violated invariant.
#include <cstdio>

#include "proof_plan.h"
#include "proof_grid.h"

using namespace kzg;

static int failures = 0;
static char case_name[96];
#define INVARIANT(c) do { if (!(c)) { ++failures; fprintf(stderr, "proof_plancheck: %s: %s\n", case_name, #c); } } while (0)

static const char* const FORM[PROOF_FORMS] = {"table", "small", "levels"};
static bool table_built[PROOF_SMALL_MAX_LOG + 1];      // the known-index table of a size is built by the first case that needs it

static void print_plan(const ProofPlan& p) {
    const size_t n = (size_t)1 << p.log_n;
    proof_print_plan(FORM[p.form], p.blocks, p.bytes_a, p.bytes_b, p.bytes_c, p.bytes_small, p.intt && n > 1, p.aux);
    if (p.form == PROOF_FORM_TABLE && !table_built[p.log_n]) {
        table_built[p.log_n] = true;
        proof_print_build((size_t)ProofStaging::zt_count(p.log_n) * 32, (size_t)PROOF_NL * n * 4, (size_t)PROOF_NL * n * 4, p.log_n);
    }
    bool unchecked = false;
    for (int i = 0; i < p.n_steps; ++i) {
        const ProofStep& s = p.step[i];
        if (unchecked && proof_step_collects_errors(s.kind)) { proof_print_check(); unchecked = false; }
        unchecked |= s.kind >= PS_FIRST_KERNEL;
        switch (s.kind) {
        case PS_UPLOAD_SCALARS: proof_print_upload_scalars(p.aux, ProofStaging::upload_bytes(p.log_n)); break;
        case PS_UPLOAD_EVALS: proof_print_upload_evals(false, n * 32); break;
        case PS_INV_SMALL: proof_print_inv_small(p.aux, p.small_lds, p.small_log_ns, p.small_out == PROOF_OUT_INV, p.small_out == PROOF_OUT_INV ? 0 : p.small_out); break;
        case PS_INV_LEVEL: {
            const ProofLevel& l = p.level[s.level];
            const uint32_t T = 1u << (l.log_l - 2);
            proof_print_inv_level(p.aux, (T + PROOF_THREADS - 1) / PROOF_THREADS, l.log_l, s.level + 1 < p.n_levels ? p.level[s.level + 1].off : p.small_out, l.off);
            break;
        }
        case PS_RECORD_CHAIN: proof_print_record(true); break;
        case PS_JOIN_CHAIN: proof_print_join(false); break;
        case PS_INVERSES: proof_print_inverses(false, p.blocks, p.next_off == PROOF_OUT_INV, p.next_off == PROOF_OUT_INV ? 0 : p.next_off, p.direct, (int)p.fused_y); break;
        case PS_FINISH_Y: proof_print_kernel("k_poly_finish_y", false, 1); break;
        case PS_READ_Y: proof_print_read_y(false, sizeof(ProofScalars)); break;
        case PS_QUOTIENT: proof_print_kernel("k_poly_quotient", false, p.blocks); break;
        case PS_QUOTIENT_ON_DOMAIN: proof_print_kernel("k_poly_quotient_on_domain", false, 1); break;
        case PS_QUOTIENT_TABLE: proof_print_kernel("k_poly_quotient_table", false, p.blocks); break;
        case PS_QUOTIENT_KNOWN: proof_print_kernel("k_poly_quotient_on_domain_known", false, 1); break;
        case PS_INTT: proof_print_intt(false); break;
        default: INVARIANT(!"a step kind");
        }
    }
    if (unchecked) proof_print_check();
    proof_end_case();
}

static void check_invariants(const ProofPlan& p, bool want, bool skip, bool z_on_domain, bool index_known, ProofEvals src) {
    const size_t n = (size_t)1 << p.log_n;
    int count[PS_KINDS] = {};
    INVARIANT(p.n_steps >= 1 && p.n_steps <= PROOF_MAX_STEPS && p.n_levels >= 0 && p.n_levels <= PROOF_MAX_LEVELS);
    for (int i = 0; i < p.n_steps; ++i) { INVARIANT(p.step[i].kind >= 0 && p.step[i].kind < PS_KINDS); ++count[p.step[i].kind]; }
    INVARIANT(p.blocks >= 1 && (size_t)p.blocks * PROOF_THREADS * PROOF_PER_LANE >= n && ((size_t)p.blocks - 1) * PROOF_THREADS * PROOF_PER_LANE < n);
    INVARIANT(p.bytes_a == (src == PROOF_EVALS_RESIDENT ? 0 : n * 32) && p.bytes_c == n * 32 && p.bytes_b == (n * PROOF_NL + p.lvl_words) * 4);
    INVARIANT(p.bytes_small == ProofStaging::PARTIALS + (size_t)p.blocks * PROOF_NL * 4 * 2);           // two sets of partial sums behind the staging head
    INVARIANT(p.intt == (want && !skip) && count[PS_INTT] == (int)p.intt && (!p.intt || p.step[p.n_steps - 1].kind == PS_INTT));
    // the evaluations go up exactly once, from a host pointer only, in front of the first kernel that reads them
    INVARIANT(count[PS_UPLOAD_EVALS] == (src == PROOF_EVALS_HOST ? 1 : 0));
    for (int i = 0, up = src != PROOF_EVALS_HOST; i < p.n_steps; ++i) {
        up |= p.step[i].kind == PS_UPLOAD_EVALS;
        if (p.step[i].kind == PS_INVERSES || p.step[i].kind == PS_QUOTIENT_TABLE) INVARIANT(up);
    }
    // the known-index form: only for a proof at a z on the domain whose index is known, 2 <= n <= 4096
    INVARIANT((p.form == PROOF_FORM_TABLE) == (index_known && want && z_on_domain && n >= 2 && n <= 4096));
    if (p.form == PROOF_FORM_TABLE) {
        INVARIANT(!p.aux && count[PS_UPLOAD_SCALARS] == 0 && count[PS_READ_Y] == 0 && count[PS_QUOTIENT_TABLE] == 1 && count[PS_QUOTIENT_KNOWN] == (p.blocks > 1 ? 1 : 0));
        INVARIANT(count[PS_INV_SMALL] + count[PS_INV_LEVEL] + count[PS_INVERSES] + count[PS_FINISH_Y] + count[PS_QUOTIENT] + count[PS_QUOTIENT_ON_DOMAIN] == 0);
        return;
    }
    INVARIANT(p.step[0].kind == PS_UPLOAD_SCALARS && count[PS_UPLOAD_SCALARS] == 1);
    INVARIANT(ProofStaging::upload_bytes(p.log_n) == ProofStaging::IMAGE_BYTES + (size_t)(2 * p.log_n + 6) * 32);      // image plus (2 log n + 6) elements
    INVARIANT(p.fused_y == (p.blocks == 1 && !z_on_domain) && count[PS_FINISH_Y] == (p.fused_y ? 0 : 1));
    INVARIANT(p.aux == (src == PROOF_EVALS_HOST && n > 512));                                            // the auxiliary stream: host evaluations and n > 2^9
    INVARIANT(count[PS_RECORD_CHAIN] == (int)p.aux && count[PS_JOIN_CHAIN] == (int)p.aux);
    INVARIANT((p.form == PROOF_FORM_SMALL) == (n <= 512) && (p.form == PROOF_FORM_SMALL) == (p.n_levels == 0 && p.small_out == PROOF_OUT_INV));
    INVARIANT(p.small_log_ns >= 0 && p.small_log_ns <= PROOF_SMALL_MAX_LOG && p.small_lds == ((size_t)PROOF_NL << p.small_log_ns) * 4 && p.small_lds <= (size_t)PROOF_NL * 4096 * 4);
    INVARIANT(count[PS_INV_SMALL] == 1 && count[PS_INV_LEVEL] == p.n_levels && count[PS_INVERSES] == 1 && count[PS_READ_Y] == 1);
    INVARIANT(count[PS_QUOTIENT] == (int)want && count[PS_QUOTIENT_ON_DOMAIN] == (want && z_on_domain ? 1 : 0) && count[PS_QUOTIENT_TABLE] + count[PS_QUOTIENT_KNOWN] == 0);
    if (p.form == PROOF_FORM_SMALL) { INVARIANT(p.direct == 1 && p.next_off == PROOF_OUT_INV && p.small_log_ns == p.log_n && p.lvl_words == 0); return; }
    // the chain: sizes n/4, n/16 .. each a quarter of the one before, the one-workgroup kernel's below them; every buffer inside the level scratch, none overlapping
    INVARIANT(p.direct == 0 && p.next_off == (p.n_levels ? p.level[0].off : p.small_out));
    int log_l = p.log_n - 2;
    size_t end = 0;
    for (int q = 0; q < p.n_levels; ++q, log_l -= 2) {
        INVARIANT(p.level[q].log_l == log_l && log_l > PROOF_CHAIN_SMALL_LOG && p.level[q].off == end);
        end += (size_t)PROOF_NL << log_l;
    }
    INVARIANT(p.small_log_ns == log_l && log_l <= PROOF_CHAIN_SMALL_LOG && log_l >= PROOF_CHAIN_SMALL_LOG - 1 && p.small_out == end);
    end += (size_t)PROOF_NL << p.small_log_ns;
    INVARIANT(end <= p.lvl_words);
    // launched coarsest first: the one-workgroup kernel, then the levels from the last to the first
    int at = 0;
    while (p.step[at].kind != PS_INV_SMALL) ++at;
    for (int q = p.n_levels - 1; q >= 0; --q) { ++at; INVARIANT(p.step[at].kind == PS_INV_LEVEL && p.step[at].level == q); }
}

int main() {
    int cases = 0;
    proof_grid([&](int log_n, bool want, bool skip, ProofGridZ zk, ProofGridSrc src) {
        ++cases;
        snprintf(case_name, sizeof case_name, "log_n=%d want=%d skip=%d z=%s src=%s", log_n, (int)want, (int)skip, PROOF_GRID_Z[zk], PROOF_GRID_SRC[src]);
        // as the driver does: the scalar table says where z lies, the index is searched only where the known-index form is open
        uint64_t z[4], zt[ProofStaging::zt_count(PROOF_MAX_LOG) * 4];
        bool z_on_domain = false;
        proof_grid_z(zk, log_n, z);
        proof_fill_scalars(z, log_n, zt, &z_on_domain);
        INVARIANT(z_on_domain == (zk != PGZ_OFF));
        uint32_t m = 0;
        const bool index_known = proof_table_eligible(log_n, want, z_on_domain) && zk == PGZ_KNOWN && kzg_host::fr_domain_index(z, log_n, &m);
        INVARIANT(!index_known || m == ((uint32_t)1 << log_n) - 1);
        const ProofEvals source = src == PGS_HOST ? PROOF_EVALS_HOST : src == PGS_SET ? PROOF_EVALS_IN_SET : PROOF_EVALS_RESIDENT;
        const ProofPlan p = proof_plan(log_n, want, skip, z_on_domain, index_known, source);
        proof_print_case(log_n, want, skip, zk, src);
        print_plan(p);
        check_invariants(p, want, skip, z_on_domain, index_known, source);
    });
    proof_end_table();
    INVARIANT(cases == PROOF_GRID_CASES);
    if (failures) fprintf(stderr, "proof_plancheck: %d invariant(s) violated\n", failures);
    return failures ? 1 : 0;
}
