// host_header_locate.h — the host side of the blob-header batch entries (capi_g2.hip: kzg_verify_length_proof_batch, kzg_header_group_sums,
// kzg_verify_length_proof_batch_locate): rows 1-4 of their error table with the two group rows behind row 4, the composite sort key of every
// G2 point, the assembly of the device's segment sums into per-group components, and the glue between those components and
// locate_search (host_locate.h): the group law on a group's components and the list of pairs its equation multiplies.
//
// For a partition of the headers into n_groups groups and the listed lengths s < n_shifts, with weights r_i and rho:
//     U_g     = sum_{i in g} r_i C_i                          (G1)
//     W_{g,s} = sum_{i in g, d_i = shift_lens[s]} r_i C2_i    (G2)
//     Pi_g    = sum_{i in g} r_i pi2_i                        (G2)
// and group g is good iff  e(U_g, G2) e(-G1, sum_s W_{g,s}) e(-[rho]G1, Pi_g) prod_s e([rho]T_s, W_{g,s}) = 1.  The equation of a union of
// groups is the same predicate on the component-wise sums, which is all locate_search needs.  Only the length classes PRESENT in the batch
// get a component: a group's sums are 2 + (classes present) points, not 2 + 64.
//
// Pure host code: no HIP type, no kzg_ctx, no device call, no curve arithmetic of its own (everything that touches a point is a template
// over the point types); also compiled with g++ by tests/hostcheck/headerlocatecheck.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "host_locate.h"

namespace kzg {

constexpr size_t HEADER_MAX_COUNT = (size_t)1 << 20;
constexpr size_t HEADER_MAX_SHIFTS = 64;
constexpr size_t HEADER_MAX_KEYS = LOCATE_MAX_GROUPS;        // n_groups (n_shifts + 1) composite keys at most

inline bool header_is_pow2(uint64_t v) { return v != 0 && (v & (v - 1)) == 0; }

// The partition of the grouped entries (on = false: the plain batch entry, no group rows)
struct HeaderGrouping {
    bool on = false;
    const uint64_t* group_indices = nullptr;
    size_t n_groups = 0;
};

// Rows 1-4 of the table of kzg_verify_length_proof_batch, in its order, then for a grouped entry the two rows its table inserts there:
//   1. handle_null (the context or an output), a null input with count > 0 (group_indices included), n_shifts = 0 with count > 0,
//      n_shifts > 64, a duplicate shift_lens entry                                                     -> KZG_ERR_INVALID_ARG
//   2. a shift_lens or claimed_lens entry that is not a power of two                                   -> KZG_ERR_NOT_POWER_OF_TWO
//   3. a claimed length that is not in shift_lens                                                      -> KZG_ERR_INVALID_ARG, *bad_index = i
//   4. count > 2^20                                                                                    -> KZG_ERR_TOO_LARGE
//   4a. a group index >= n_groups, or n_groups = 0 with count > 0                                      -> KZG_ERR_INVALID_ARG
//   4b. n_groups (n_shifts + 1) > 2^28                                                                 -> KZG_ERR_TOO_LARGE
// Nothing is allocated before row 4 has passed.  length_class[i] = the position of claimed_lens[i] in shift_lens.
inline int32_t header_batch_checks(bool handle_null, const void* commitments, const void* length_commitments, const void* length_proofs,
                                   const uint64_t* claimed_lens, size_t count, const uint64_t* shift_lens, const void* g1_tau_shifts, size_t n_shifts,
                                   const HeaderGrouping& grp, std::vector<uint8_t>* length_class, uint64_t* bad_index) {
    if (handle_null) return KZG_ERR_INVALID_ARG;
    if (count && (!commitments || !length_commitments || !length_proofs || !claimed_lens || !shift_lens || !g1_tau_shifts || n_shifts == 0)) return KZG_ERR_INVALID_ARG;
    if (count && grp.on && !grp.group_indices) return KZG_ERR_INVALID_ARG;
    if (n_shifts > HEADER_MAX_SHIFTS || (n_shifts && (!shift_lens || !g1_tau_shifts))) return KZG_ERR_INVALID_ARG;
    for (size_t g = 0; g < n_shifts; ++g)
        for (size_t h = 0; h < g; ++h) if (shift_lens[g] == shift_lens[h]) return KZG_ERR_INVALID_ARG;
    for (size_t g = 0; g < n_shifts; ++g) if (!header_is_pow2(shift_lens[g])) return KZG_ERR_NOT_POWER_OF_TWO;
    for (size_t i = 0; i < count; ++i) if (!header_is_pow2(claimed_lens[i])) return KZG_ERR_NOT_POWER_OF_TWO;
    int8_t class_of_log[64];
    memset(class_of_log, -1, sizeof class_of_log);
    for (size_t g = 0; g < n_shifts; ++g) class_of_log[__builtin_ctzll(shift_lens[g])] = (int8_t)g;
    for (size_t i = 0; i < count; ++i)
        if (class_of_log[__builtin_ctzll(claimed_lens[i])] < 0) { if (bad_index) *bad_index = (uint64_t)i; return KZG_ERR_INVALID_ARG; }
    if (count > HEADER_MAX_COUNT) return KZG_ERR_TOO_LARGE;
    if (grp.on) {
        const int32_t rc = locate_check_groups(grp.group_indices, count, grp.n_groups);
        if (rc != KZG_OK) return rc;
        if (grp.n_groups > HEADER_MAX_KEYS / (n_shifts + 1)) return KZG_ERR_TOO_LARGE;
    }
    length_class->resize(count);
    for (size_t i = 0; i < count; ++i) (*length_class)[i] = (uint8_t)class_of_log[__builtin_ctzll(claimed_lens[i])];
    return KZG_OK;
}

// The sort key of every G2 point, in the order of the upload (point 2 i = C2_i, point 2 i + 1 = pi2_i):
//     C2_i  -> g n_shifts + s               (group g, length class s)
//     pi2_i -> n_groups n_shifts + g
// so that locate_plan on these 2 count keys (header_n_keys of them possible) puts every W_{g,s} and every Pi_g into a segment of its own.
inline size_t header_n_keys(size_t n_groups, size_t n_shifts) { return n_groups * (n_shifts + 1); }
inline void header_locate_keys(const uint64_t* group_indices, const uint8_t* length_class, size_t count, size_t n_groups, size_t n_shifts, std::vector<uint64_t>* keys) {
    keys->resize(2 * count);
    for (size_t i = 0; i < count; ++i) {
        (*keys)[2 * i] = group_indices[i] * n_shifts + length_class[i];
        (*keys)[2 * i + 1] = n_groups * n_shifts + group_indices[i];
    }
}

// The length classes some header of the batch claims, ascending: slot_of[s] = the position of class s among them, or -1
struct HeaderClasses {
    std::vector<int32_t> slot_of;      // n_shifts entries
    std::vector<uint32_t> present;
};
inline HeaderClasses header_present_classes(const uint8_t* length_class, size_t count, size_t n_shifts) {
    HeaderClasses c;
    c.slot_of.assign(n_shifts, -1);
    for (size_t i = 0; i < count; ++i) c.slot_of[length_class[i]] = 0;
    for (size_t s = 0; s < n_shifts; ++s)
        if (c.slot_of[s] == 0) { c.slot_of[s] = (int32_t)c.present.size(); c.present.push_back((uint32_t)s); }
    return c;
}

// The components of a group, or of a sum of groups: u = U, q[0] = Pi, q[1 + c] = W of the c-th PRESENT class.  A missing q entry is the
// identity, so that a value may carry the G1 side alone (q empty) or the G2 side alone (u the identity): locate_search sums its `lhs` and
// `rhs` arrays separately, and the leaves put U into lhs and the G2 components into rhs.
template <class A, class B>
struct HeaderSums {
    A u;
    std::vector<B> q;
};

// The group law on such values from the laws OA on A and OB on B (each: zero(), add(x, y), sub(x, y)): the Ops of locate_search
template <class A, class B, class OA, class OB>
struct HeaderSumOps {
    OA oa;
    OB ob;
    using P = HeaderSums<A, B>;
    P zero() const { return P{oa.zero(), {}}; }
    P combine(const P& a, const P& b, bool minus) const {
        P r;
        r.u = minus ? oa.sub(a.u, b.u) : oa.add(a.u, b.u);
        const size_t n = a.q.size() > b.q.size() ? a.q.size() : b.q.size();
        r.q.reserve(n);
        for (size_t k = 0; k < n; ++k) {
            const B x = k < a.q.size() ? a.q[k] : ob.zero(), y = k < b.q.size() ? b.q[k] : ob.zero();
            r.q.push_back(minus ? ob.sub(x, y) : ob.add(x, y));
        }
        return r;
    }
    P add(const P& a, const P& b) const { return combine(a, b, false); }
    P sub(const P& a, const P& b) const { return combine(a, b, true); }
};

// The leaves of the search from the device's segment sums.  g1_plan: locate_plan of the headers by group (segment j = group
// g1_plan.segs[j], its sum u_of(j)); g2_plan: locate_plan of the 2 count keys above (segment j = key g2_plan.segs[j], its sum q_of(j)).
// An empty group, and a class no header of a group claims, keep the identities zero_a / zero_b.
template <class A, class B, class UOf, class QOf>
void header_assemble(const LocatePlan& g1_plan, const LocatePlan& g2_plan, size_t n_groups, size_t n_shifts, const HeaderClasses& cls, const UOf& u_of,
                     const QOf& q_of, const A& zero_a, const B& zero_b, std::vector<HeaderSums<A, B>>* lhs, std::vector<HeaderSums<A, B>>* rhs) {
    lhs->assign(n_groups, HeaderSums<A, B>{zero_a, {}});
    rhs->assign(n_groups, HeaderSums<A, B>{zero_a, std::vector<B>(1 + cls.present.size(), zero_b)});
    for (size_t j = 0; j < g1_plan.segs.size(); ++j) (*lhs)[g1_plan.segs[j]].u = u_of(j);
    const size_t n_w = n_groups * n_shifts;
    for (size_t j = 0; j < g2_plan.segs.size(); ++j) {
        const size_t key = g2_plan.segs[j];
        if (key < n_w) (*rhs)[key / n_shifts].q[1 + (size_t)cls.slot_of[key % n_shifts]] = q_of(j);
        else (*rhs)[key - n_w].q[0] = q_of(j);
    }
}

// What the equation multiplies, the same for every test of a call: G2, -G1, -[rho]G1 and [rho]T_s for the present classes (rho stands on
// the G1 side: e(-[rho]G1, Pi) is e(-G1, [rho]Pi), and [rho]T_s is needed anyway, so no test multiplies a G2 point by rho)
template <class P1, class P2>
struct HeaderFixed {
    P2 g2;
    P1 neg_g1, neg_rho_g1;
    std::vector<P1> rho_shift;         // per present class
};
// The pairs of the equation of a sum with components u (G1) and q (Pi, then W per present class); sum_w = the sum of those W.
// prod_k e(ps[k], qs[k]) = 1 iff the sum is good.
template <class P1, class P2>
void header_pairs(const HeaderFixed<P1, P2>& fx, const P1& u, const std::vector<P2>& q, const P2& sum_w, std::vector<P1>* ps, std::vector<P2>* qs) {
    ps->clear(); qs->clear();
    ps->push_back(u); qs->push_back(fx.g2);
    ps->push_back(fx.neg_g1); qs->push_back(sum_w);
    ps->push_back(fx.neg_rho_g1); qs->push_back(q[0]);
    for (size_t c = 0; c + 1 < q.size(); ++c) { ps->push_back(fx.rho_shift[c]); qs->push_back(q[1 + c]); }
}

}  // namespace kzg
