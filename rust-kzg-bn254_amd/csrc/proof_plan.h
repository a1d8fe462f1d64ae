// proof_plan.h — the policy of the proof driver (poly.hip proof_enqueue) and the layout of its staging memory: from log n, what is wanted, where z
// lies and where the evaluations are to everything the driver decides before its first launch -- the form of the inversion chain, the grids, the
// level buffers, the workspace bytes, the streams and the ordered list of launches -- plus the table of scalars the host computes for the chain.
// Pure host code over host_fr.h: no HIP type, no kzg_ctx, no allocation; also compiled with g++ by tests/hostcheck/proof_plancheck.cpp, which pins
// every plan of a fixed grid (tests/golden/proof_plans.txt), and by tests/hostcheck/proof_scalars.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "host_fr.h"
#include "host_log2.h"

namespace kzg {

constexpr int PROOF_NL = 9;                  // limbs of a device Fr (field29.h NL; poly.hip asserts the two are one number)
constexpr int PROOF_THREADS = 256;           // workgroup of the per-element kernels (poly_common.h POLY_THREADS)
constexpr int PROOF_PER_LANE = 4;            // elements per lane of the last inversion level = its coset size (k_poly_inverses)
constexpr int PROOF_SMALL_MAX_LOG = 12;      // the one-workgroup kernel holds up to 2^12 inverses in LDS (poly.hip POLY_SMALL_MAX_LOG)
constexpr int PROOF_MAX_LOG = 28;            // the largest domain
// The one-workgroup kernel takes the chain up to 2^chain_small_log points, x4 levels on the whole chip go on from there: its late levels
// keep all 16 waves of one CU busy, a x4 launch over many CUs costs about one of them.  Chain lengths 2..12, off-domain proofs of
// 2^11 / 2^12 / 2^14 evaluations (same box; measured with tools/archive/time_proof_sizes.py on a build with this constant read from the
// environment, a switch that is gone): 12 -> 0.231 / 0.295 / 0.426 ms, 9 -> 0.226 / 0.281 / 0.414, 7 -> 0.230 / 0.286 / 0.422
constexpr int PROOF_CHAIN_SMALL_LOG = 9;
static_assert(PROOF_CHAIN_SMALL_LOG >= 2 && PROOF_CHAIN_SMALL_LOG <= PROOF_SMALL_MAX_LOG, "the one-workgroup kernel holds the chain's first levels in LDS");
constexpr int PROOF_MAX_LEVELS = (PROOF_MAX_LOG - 2 - PROOF_CHAIN_SMALL_LOG + 1) / 2;      // x4 levels of the largest domain: 2^26, 2^24 .. 2^10

struct ProofScalars {        // device-resident small state of one proof computation
    uint32_t on_domain_index; // NO_INDEX if z is not a domain element
    uint32_t pad[3];
    int32_t y[PROOF_NL];      // y = p(z), internal form, reduced
    uint32_t y_wire[8];
};

// Staging of one proof: PolySet::pinned (host, PINNED_BYTES) and the head of PolySet::small (device) share one layout, so that one copy
// pinned -> small brings up the image and the chain's scalars.
struct ProofStaging {
    static constexpr size_t IMAGE = 0;            // both: the initial ProofScalars (index NO_INDEX, the rest zero), zero-filled to IMAGE_BYTES
    static constexpr size_t IMAGE_BYTES = 1024;
    static constexpr size_t ZT = IMAGE + IMAGE_BYTES;   // both: zt, the scalars of the inversion chain, 32-byte wire elements (indices below)
    static constexpr size_t Y_READBACK = 3072;    // pinned: the ProofScalars the kernels leave (copied back, or written in place by the table form)
    static constexpr size_t PINNED_BYTES = 4096;
    static constexpr size_t PARTIALS = 4096;      // small: two sets of per-workgroup partial sums, PROOF_NL planes each
    // zt[a] = z^(2^a) for a <= log_n; zt[log_n + 1] = 1 / (1 - z^n) (zero: z on the domain); and, read only when z is on the domain,
    // zt[log_n + 2 + a] = z^-(2^a) for a <= log_n and zt[2 log_n + 3 ..] = 1/(i - 1), -1/2, 1/(-i - 1)
    static constexpr int zt_pow(int a) { return a; }
    static constexpr int zt_top(int log_n) { return log_n + 1; }
    static constexpr int zt_inv_pow(int log_n, int a) { return log_n + 2 + a; }
    static constexpr int zt_const(int log_n, int k) { return 2 * log_n + 3 + k; }
    static constexpr int zt_count(int log_n) { return 2 * log_n + 6; }
    static constexpr size_t upload_bytes(int log_n) { return IMAGE_BYTES + (size_t)zt_count(log_n) * 32; }      // the one copy pinned -> small
    static constexpr size_t small_bytes(uint32_t blocks) { return PARTIALS + (size_t)blocks * PROOF_NL * 4 * 2; }
};
static_assert(sizeof(ProofScalars) <= ProofStaging::IMAGE_BYTES, "the ProofScalars image and the zt table are uploaded as one block");
static_assert(ProofStaging::upload_bytes(0) == ProofStaging::IMAGE_BYTES + 6 * 32 && ProofStaging::ZT == ProofStaging::IMAGE + ProofStaging::IMAGE_BYTES,
              "the upload covers exactly the image and the scalars behind it");
static_assert(ProofStaging::ZT + (size_t)ProofStaging::zt_count(PROOF_MAX_LOG) * 32 <= ProofStaging::Y_READBACK, "the scalars of the largest domain end below the y read-back slot");
static_assert(ProofStaging::upload_bytes(PROOF_MAX_LOG) <= ProofStaging::PARTIALS, "... and below the partial sums");
static_assert(ProofStaging::Y_READBACK + sizeof(ProofScalars) <= ProofStaging::PINNED_BYTES, "the read-back slot holds a ProofScalars");
static_assert(ProofStaging::zt_const(PROOF_MAX_LOG, 3) == ProofStaging::zt_count(PROOF_MAX_LOG), "three constants end the table");

// The chain's scalars for the point z (wire) on the 2^log_n-point domain: zt_count(log_n) wire elements; *z_on_domain = (z^n == 1).
inline void proof_fill_scalars(const uint64_t z[4], int log_n, uint64_t* zt, bool* z_on_domain) {
    memcpy(zt, z, 32);
    for (int a = 1; a <= log_n; ++a) kzg_host::fr_mul(zt + 4 * (a - 1), zt + 4 * (a - 1), zt + 4 * a);
    const uint64_t one_int[4] = {1, 0, 0, 0};
    uint64_t one_w[4], den[4];
    kzg_host::fr_mul(kzg_host::FR_R2, one_int, one_w);
    kzg_host::fr_sub(one_w, zt + 4 * log_n, den);                // 1 - z^n (zero: z is on the domain, the device inverts what it needs itself)
    uint64_t* top = zt + 4 * ProofStaging::zt_top(log_n);
    uint64_t* zit = zt + 4 * ProofStaging::zt_inv_pow(log_n, 0);  // z^-(2^a), a <= log_n: only read when z is on the domain
    uint64_t* cst = zt + 4 * ProofStaging::zt_const(log_n, 0);    // 1/(i - 1), -1/2, 1/(-i - 1), i = w^(n/4) = 5^((r-1)/4)
    *z_on_domain = (den[0] | den[1] | den[2] | den[3]) == 0;
    if (*z_on_domain) {
        memset(top, 0, 32);
        kzg_host::fr_inv(zt, zit);
        for (int a = 1; a <= log_n; ++a) kzg_host::fr_mul(zit + 4 * (a - 1), zit + 4 * (a - 1), zit + 4 * a);
    } else {
        kzg_host::fr_inv(den, top);
        memset(zit, 0, (size_t)(log_n + 1) * 32);
    }
    memcpy(cst, kzg_host::fr_on_domain_constants(), 96);
}

enum ProofEvals { PROOF_EVALS_HOST, PROOF_EVALS_IN_SET, PROOF_EVALS_RESIDENT };   // a host pointer; already in set.a; in a device buffer of the caller's
enum ProofForm {
    PROOF_FORM_TABLE,             // z = w^m with m known on a small domain: the inverses come from the domain's table 1 / (w^k - 1)
    PROOF_FORM_SMALL,             // the one-workgroup kernel gives all n inverses' coarser level
    PROOF_FORM_LEVELS,            // the one-workgroup kernel, then x4 levels up to n / 4
    PROOF_FORMS
};
enum ProofStepKind {
    PS_UPLOAD_SCALARS,            // pinned -> small: image + zt, on the chain's stream
    PS_UPLOAD_EVALS,              // host evaluations -> set.a, on the main stream
    PS_RECORD_CHAIN,              // an event behind the chain on the auxiliary stream ...
    PS_JOIN_CHAIN,                // ... for which the main stream waits
    PS_READ_Y,                    // small -> pinned: the ProofScalars with y
    PS_INTT,                      // ntt_run: the quotient's coefficients
    PS_INV_SMALL,                 // the kernels: k_poly_inv_small
    PS_INV_LEVEL,                 // k_poly_inv_level of level[.level]
    PS_INVERSES,                  // k_poly_inverses
    PS_FINISH_Y,                  // k_poly_finish_y
    PS_QUOTIENT,                  // k_poly_quotient
    PS_QUOTIENT_ON_DOMAIN,        // k_poly_quotient_on_domain
    PS_QUOTIENT_TABLE,            // k_poly_quotient_table
    PS_QUOTIENT_KNOWN,            // k_poly_quotient_on_domain_known
    PS_KINDS,
    PS_FIRST_KERNEL = PS_INV_SMALL
};
struct ProofStep { int kind, level; };
// launch errors (hipGetLastError) are collected in front of these steps, if a kernel was launched since the last time, and behind the last step
inline bool proof_step_collects_errors(int kind) { return kind == PS_RECORD_CHAIN || kind == PS_READ_Y || kind == PS_INTT; }
struct ProofLevel {
    int log_l;                    // the level's domain has 2^log_l points
    size_t off;                   // its inverses: word offset inside the level scratch (behind the n inverses in set.b)
};
constexpr size_t PROOF_OUT_INV = ~(size_t)0;      // "the n inverses at the head of set.b" where a level-scratch offset is expected
constexpr int PROOF_MAX_STEPS = PROOF_MAX_LEVELS + 13;

struct ProofPlan {
    int log_n;
    int form;                     // ProofForm
    uint32_t blocks;              // workgroups of the per-element kernels
    bool fused_y;                 // one workgroup holds the whole barycentric sum: no second launch for y
    int small_log_ns;             // the one-workgroup kernel: size of its domain, ...
    size_t small_lds;             // ... dynamic LDS bytes, ...
    size_t small_out;             // ... and where it writes: a level-scratch word offset, or PROOF_OUT_INV
    int n_levels;
    ProofLevel level[PROOF_MAX_LEVELS];      // largest first; launched last to first, each reading the one after it (the last: small_out)
    size_t next_off;              // what k_poly_inverses reads as the coarser level (level-scratch offset or PROOF_OUT_INV) ...
    int direct;                   // ... and whether that already is the finest level (the small form)
    size_t lvl_words;             // the level scratch
    size_t bytes_a, bytes_b, bytes_c, bytes_small;
    bool aux;                     // the chain runs on the auxiliary stream, while the host sits in the upload of the evaluations on the main one
    bool intt;                    // an inverse NTT of the quotient follows (its tables are needed when n > 1)
    int n_steps;
    ProofStep step[PROOF_MAX_STEPS];
};

// the known-index form is open to: a proof, z on the domain, 2 <= n <= 4096 (compute_proof_with_known_z_fr_index at the reference's bench sizes);
// the driver then looks for the index (host_fr.h fr_domain_index) and passes what it found as index_known
inline bool proof_table_eligible(int log_n, bool want_proof, bool z_on_domain) { return want_proof && z_on_domain && log_n >= 1 && log_n <= PROOF_SMALL_MAX_LOG; }

inline ProofPlan proof_plan(int log_n, bool want_proof, bool skip_intt, bool z_on_domain, bool index_known, ProofEvals evals) {
    ProofPlan p{};
    const size_t n = (size_t)1 << log_n;
    p.log_n = log_n;
    // lanes of the last level: 4 elements each (one coset), at least one block
    p.blocks = (uint32_t)((n + (size_t)PROOF_THREADS * PROOF_PER_LANE - 1) / ((size_t)PROOF_THREADS * PROOF_PER_LANE));
    const size_t chain_small_max = (size_t)1 << PROOF_CHAIN_SMALL_LOG;
    const size_t n1 = n > chain_small_max ? n / 4 : 0;       // the level above the last one (0: the small kernel gives all n inverses)
    p.lvl_words = n1 ? (n1 + n1 / 2) * PROOF_NL + 64 : 0;     // sum over n/4, n/16, ... < n1 * 4/3
    p.bytes_a = evals == PROOF_EVALS_RESIDENT ? 0 : n * 32;  // evaluations (wire)
    p.bytes_b = (n * PROOF_NL + p.lvl_words) * 4;            // inverses (planes) | level scratch: the smaller domains' inverses
    p.bytes_c = n * 32;                                      // quotient (wire)
    p.bytes_small = ProofStaging::small_bytes(p.blocks);
    p.intt = want_proof && !skip_intt;                       // commit_eval_form(quotient): coefficients = IFFT(q), then MSM over the monomial SRS (kzg.rs:176-177)
    const bool host_evals = evals == PROOF_EVALS_HOST;
    auto push = [&p](int kind, int level = 0) { p.step[p.n_steps].kind = kind; p.step[p.n_steps].level = level; ++p.n_steps; };
    if (index_known && proof_table_eligible(log_n, want_proof, z_on_domain)) {
        // (no upload of the ProofScalars image and no copy back: the kernels only WRITE it, straight into the pinned read-back slot)
        p.form = PROOF_FORM_TABLE;
        if (host_evals) push(PS_UPLOAD_EVALS);
        push(PS_QUOTIENT_TABLE);
        if (p.blocks > 1) push(PS_QUOTIENT_KNOWN);
        if (p.intt) push(PS_INTT);
        return p;
    }
    // The chain needs z only, not the evaluations: for a proof from HOST evaluations it is enqueued FIRST, on the context's auxiliary stream, and
    // runs while this thread is inside the pageable upload of the evaluations (0.6 ms at 2^20; the chain: six launches, ~0.09 ms of latency).
    p.aux = host_evals && n > chain_small_max;
    p.fused_y = p.blocks == 1 && !z_on_domain;
    push(PS_UPLOAD_SCALARS);
    if (host_evals && !p.aux) push(PS_UPLOAD_EVALS);
    // the chain of smaller domains, coarsest first: small kernel (<= 4096 points, in LDS), then x4 levels, then the last level
    if (n <= chain_small_max) {
        p.form = PROOF_FORM_SMALL;
        p.small_log_ns = log_n;
        p.small_out = p.next_off = PROOF_OUT_INV;
        p.direct = 1;
        push(PS_INV_SMALL);
    } else {
        p.form = PROOF_FORM_LEVELS;
        size_t cursor = 0;
        int log_l = log_n - 2;                               // sizes n/4, n/16, .. down to the first one <= 2^chain_small_log
        for (; log_l > PROOF_CHAIN_SMALL_LOG; log_l -= 2) {
            p.level[p.n_levels].log_l = log_l;
            p.level[p.n_levels].off = cursor;
            cursor += (size_t)PROOF_NL << log_l;
            ++p.n_levels;
        }
        p.small_log_ns = log_l;
        p.small_out = cursor;
        push(PS_INV_SMALL);
        for (int q = p.n_levels - 1; q >= 0; --q) push(PS_INV_LEVEL, q);
        p.next_off = p.n_levels ? p.level[0].off : p.small_out;
        if (p.aux) { push(PS_RECORD_CHAIN); push(PS_UPLOAD_EVALS); push(PS_JOIN_CHAIN); }   // the upload of the evaluations now (the host sits in it while the chain runs), then join
    }
    p.small_lds = ((size_t)PROOF_NL << p.small_log_ns) * 4;
    push(PS_INVERSES);
    if (!p.fused_y) push(PS_FINISH_Y);
    push(PS_READ_Y);
    if (!want_proof) return p;
    push(PS_QUOTIENT);
    if (z_on_domain) push(PS_QUOTIENT_ON_DOMAIN);            // (z off the domain: the kernel would return at once)
    if (p.intt) push(PS_INTT);
    return p;
}

}  // namespace kzg
