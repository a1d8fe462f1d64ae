// host_prove_cosets.h — the host side of kzg_prove_cosets / kzg_coset_quotients (provecosets.hip, capi_prove.hip): every argument check of the
// entries in the order the header documents, and everything the driver decides before its first launch -- the segment length S, the levels
// of the carry recursion, the launches of a group, the bytes an item and a group reserve, the groups of a call -- plus the index arithmetic
// the kernels share with the host model of tests/hostcheck/provecosetscheck.cpp.  Pure host code: no HIP type, no kzg_ctx, no allocation.
//
// The proof of coset k of f (deg f < d, chunk length l, D = d / l, c = w^(k l)) is [q(tau)]_1 with f = q (X^l - c) + r.  Per residue
// rho < l the coefficients a_t = f_(rho + t l), t < D, form one CHAIN: G_t = a_t + c G_(t+1), G_D = 0 (a suffix Horner sum).  Then
//   q_(rho + (t-1) l) = G_t for 1 <= t < D,   q_(rho + (D-1) l) = 0,   r_rho = G_0
// (g_s = G_(s+1) is the same recurrence indexed by the quotient coefficient).  A chain is cut into segments of S elements, t in [j S, (j+1) S): the segment's own Horner sum
// with zero carry-in is loc_t, its head is loc_(j S), and
//   G_t = loc_t + c^((j+1) S - t) G_((j+1) S),        G_(j S) = head_j + c^S G_((j+1) S).
// The second line is the same recurrence on the heads with the multiplier c^S: LEVEL i of the recursion runs the local pass on the heads
// of level i - 1 with the multiplier c^(S^i), until a level is one segment; the fix-up passes then walk back down.  Every c^e is a domain
// element w^(k l S^i e mod n): no power table.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/kzg_bn254_mi355x.h"
#include "host_encode.h"

#if defined(__HIPCC__)
#define KZG_PC_HD __host__ __device__ __forceinline__
#else
#define KZG_PC_HD inline
#endif

namespace kzg {

constexpr uint32_t PROVE_SEG = 64;                 // S: the dependent products of a lane in one pass (a shorter chain is one segment)
constexpr int PROVE_MAX_LEVELS = 6;                // D <= 2^23 and S = 64 need 4
constexpr size_t PROVE_GROUP_MAX = 32768;          // items per group: grid.y of a launch (< 65 536)
constexpr size_t PROVE_ITEM_INDEX_BYTES = 8;       // polynomial slot and coset index of an item, one u32 each
// THE RULE for a group of one item (tools/time_prove_cosets.py, profiles/prove_cosets.md): its quotient goes through msm_run, the
// single commitment of the library, instead of the batched bucket problem of commit_batch_device; two items or more are one batch.
constexpr size_t PROVE_MSM_SINGLE_MAX_ITEMS = 1;

// ---- index arithmetic shared by the kernels and the host model ------------------------------------------------------------------------
// the exponent E of c_i = c^(S^i) = w^E: shift = log2(l S^i), mask = n - 1
KZG_PC_HD uint32_t pc_mult_exp(uint32_t k, int shift, uint32_t mask) { return (uint32_t)(((uint64_t)k << shift) & mask); }
// the exponent of c_i^e
KZG_PC_HD uint32_t pc_pow_exp(uint32_t k, int shift, uint32_t e, uint32_t mask) { return (uint32_t)(((uint64_t)pc_mult_exp(k, shift, mask) * e) & mask); }
// the exponent of the twist w^(k rho) of remainder coefficient rho
KZG_PC_HD uint32_t pc_twist_exp(uint32_t k, uint32_t rho, uint32_t mask) { return (uint32_t)(((uint64_t)k * rho) & mask); }
// element j of chain rho inside a row of a level (the polynomial, a quotient row's source, the heads): chains interleaved, as in f
KZG_PC_HD size_t pc_elem(uint32_t j, uint32_t l, uint32_t rho) { return (size_t)j * l + rho; }
// where level 0 keeps loc_t / G_t, t >= 1, in the quotient row: the place of q_(rho + (t-1) l)
KZG_PC_HD size_t pc_quot_elem(uint32_t t, uint32_t l, uint32_t rho) { return (size_t)(t - 1) * l + rho; }

// ---- the checks -------------------------------------------------------------------------------------------------------------------------
// Checks 1 and 2 of the header's table are `bad_pointers` (with count == 0) and `bad_srs`; check 3 is rows 3 .. 6 of kzg_encode_cosets'
// table (encode_check; kzg_coset_quotients and the query pass srs_len = SIZE_MAX: no row 6).
inline int32_t prove_cosets_check_shape(bool bad_pointers, bool bad_srs, size_t count, size_t poly_len, size_t n, size_t chunk_len, size_t srs_len) {
    return encode_check(bad_pointers || count == 0, bad_srs, poly_len, n, chunk_len, srs_len);
}
// Check 4: a polynomial index >= count or a coset index >= m; *bad = the smallest such item
inline int32_t prove_cosets_check_items(const uint64_t* poly_indices, const uint64_t* coset_indices, size_t n_items, size_t count, size_t m, uint64_t* bad) {
    for (size_t i = 0; i < n_items; ++i)
        if ((poly_indices && poly_indices[i] >= count) || coset_indices[i] >= m) { if (bad) *bad = i; return KZG_ERR_INVALID_ARG; }
    return KZG_OK;
}
// Check 5: the polynomials (count x d x 32 bytes) and the largest output row (a quotient: d x 32 bytes; else max(l x 32, 64)) times
// n_items must fit size_t
inline int32_t prove_cosets_check_sizes(size_t count, size_t poly_len, size_t chunk_len, size_t n_items, bool quotients) {
    if (count > SIZE_MAX / (poly_len * ENCODE_FR_BYTES)) return KZG_ERR_INVALID_ARG;
    const size_t row = quotients ? poly_len * ENCODE_FR_BYTES : std::max(chunk_len * ENCODE_FR_BYTES, ENCODE_AFFINE_BYTES);
    if (n_items > SIZE_MAX / row) return KZG_ERR_INVALID_ARG;
    return KZG_OK;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------------------
struct ProveLevel {
    uint32_t len = 0;        // elements of a chain at this level: D at level 0, the segments of the level below above it
    uint32_t nseg = 0;       // its segments: ceil(len / S)
    int shift = 0;           // log2(l S^level): the level's multiplier is w^((k << shift) mod n)
    bool heads = false;      // its local pass writes the segment heads (level 0 always: head 0 is the remainder)
    size_t data_off = 0;     // level >= 1: where the level's elements (= the heads of the level below) start in an item's heads block, in elements
    size_t heads_off = 0;    // where its own heads start there
};

struct ProveCosetsPlan {
    size_t d = 0, n = 0, l = 0, D = 0, m = 0;
    int log_d = 0, log_n = 0, log_l = 0, log_S = 0;
    bool values = false, quotients = false;       // quotients: the rows are kept (for the proofs, or as the output)
    uint32_t S = 0;
    int n_levels = 0;                              // local passes: 1 + carry levels
    ProveLevel level[PROVE_MAX_LEVELS];
    size_t heads_elems = 0;                        // elements of an item's heads block (every level's heads, one after the other)
    size_t ntt_bytes[2] = {0, 0};                  // per item: the workspace of its l-point transform (0 up to l = 1024: one pass in place)
    size_t item_bytes = 0;                         // quotient row + heads + remainder + transform workspace + indices
    size_t n_items = 0, budget = 0;
    size_t group = 1, n_groups = 0, group_bytes = 0;
    bool msm_single = false;                       // a full group is one item and its proof goes through msm_run
    uint32_t launches = 0;                         // kernel launches of a group on the Fr side: local and fix-up passes, the passes of the transform
    int carry_levels() const { return n_levels - 1; }
    int fixups() const { return n_levels >= 2 ? n_levels - 2 : 0; }    // the fix-up passes above level 0 (the top level is final as it is)
};

// The levels of the carry recursion for chains of p.D elements cut into segments of S (a power of two): level 0 is the chain, level i + 1
// the heads of level i, until a level is one segment.  (The planner's S is min(D, PROVE_SEG); the host model also runs smaller ones.)
inline void prove_cosets_set_levels(ProveCosetsPlan& p, uint32_t S) {
    p.S = S;
    p.log_S = g1fft_log2(S);
    size_t len = p.D, off = 0;
    for (int i = 0; i < PROVE_MAX_LEVELS; ++i) {
        ProveLevel& L = p.level[i];
        L.len = (uint32_t)len;
        L.nseg = (uint32_t)((len + S - 1) / S);
        L.shift = p.log_l + i * p.log_S;
        L.heads = i == 0 || L.nseg > 1;
        L.data_off = i == 0 ? 0 : p.level[i - 1].heads_off;
        L.heads_off = off;
        if (L.heads) off += (size_t)L.nseg * p.l;
        p.n_levels = i + 1;
        if (L.nseg == 1) break;
        len = L.nseg;
    }
    p.heads_elems = off;
}

// The plan of a call whose arguments passed the checks.  group_bytes = 0: the default budget (ENCODE_GROUP_BYTES_DEFAULT).
inline ProveCosetsPlan prove_cosets_plan(size_t poly_len, size_t n, size_t chunk_len, size_t n_items, bool values, bool quotients, size_t group_bytes) {
    ProveCosetsPlan p;
    p.d = poly_len; p.n = n; p.l = chunk_len; p.D = poly_len / chunk_len; p.m = n / chunk_len;
    p.log_d = g1fft_log2(p.d); p.log_n = g1fft_log2(n); p.log_l = g1fft_log2(p.l);
    p.values = values; p.quotients = quotients;
    prove_cosets_set_levels(p, (uint32_t)std::min<size_t>(p.D, PROVE_SEG));
    if (values && p.log_l >= 1) {
        const NttPlan np = ntt_plan(p.log_l, false, 256, 0);
        p.ntt_bytes[0] = np.bytes_data; p.ntt_bytes[1] = np.bytes_tmp;
        p.launches += (uint32_t)np.n_passes;
    }
    p.launches += (uint32_t)p.n_levels + (uint32_t)p.fixups() + 1u;
    p.item_bytes = (quotients ? p.d : 0) * ENCODE_FR_BYTES + p.heads_elems * ENCODE_FR_BYTES + (values ? p.l * ENCODE_FR_BYTES : 0) +
                   p.ntt_bytes[0] + p.ntt_bytes[1] + PROVE_ITEM_INDEX_BYTES;
    p.n_items = n_items;
    p.budget = group_bytes ? group_bytes : ENCODE_GROUP_BYTES_DEFAULT;
    p.group = std::max<size_t>(1, std::min(std::min(std::max<size_t>(n_items, 1), PROVE_GROUP_MAX), p.budget / p.item_bytes));
    p.n_groups = (n_items + p.group - 1) / p.group;
    p.group_bytes = p.group * p.item_bytes;
    p.msm_single = p.group <= PROVE_MSM_SINGLE_MAX_ITEMS;
    return p;
}

}  // namespace kzg
