// host_locate.h — the host side of kzg_coset_group_sums / kzg_verify_multiproof_batch_locate (multilocate.hip, capi_coset.hip): the checks
// of the group arguments in the order the header documents, the stable counting sort of the items by group (a permutation and segment
// offsets: the values themselves are never reordered), and the search of the tree of group sums for the bad groups.
// Pure host code: no HIP type, no kzg_ctx, no device call, no curve arithmetic of its own (the search is a template over the point type
// and the predicate); also compiled with g++ by tests/hostcheck/locatecheck.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/kzg_bn254_mi355x.h"

namespace kzg {

constexpr size_t LOCATE_MAX_GROUPS = (size_t)1 << 28;
constexpr uint32_t LOCATE_WAVE = 64;         // lanes whose points the device sums before it leaves a partial (multilocate.hip)

// check 2 of the header's table: every group index below n_groups (so n_groups = 0 with count > 0 fails on the first item)
inline int32_t locate_check_groups(const uint64_t* group_indices, size_t count, size_t n_groups) {
    for (size_t i = 0; i < count; ++i)
        if (group_indices[i] >= n_groups) return KZG_ERR_INVALID_ARG;
    return KZG_OK;
}

struct LocatePlan {
    size_t count = 0, n_groups = 0;
    std::vector<uint32_t> perm;        // [sorted position] -> item; items of one group keep the caller's order (stable): count entries
    std::vector<uint32_t> offsets;     // group g owns the sorted positions [offsets[g], offsets[g + 1]): n_groups + 1 entries
    // what the device is given: the NON-EMPTY groups only, so that nothing there grows with n_groups
    std::vector<uint32_t> segs;        // the non-empty groups, ascending
    std::vector<uint32_t> seg_off;     // segment j = group segs[j] owns the sorted positions [seg_off[j], seg_off[j + 1]): segs.size() + 1 entries
    std::vector<uint32_t> seg_of;      // [sorted position] -> its segment: count entries
    // a wave of LOCATE_WAVE consecutive sorted positions leaves one partial sum per segment it touches; those of segment j are the slots
    // [part_off[j], part_off[j + 1]), the wave w (= position / LOCATE_WAVE) at slot part_off[j] + w - seg_off[j] / LOCATE_WAVE
    std::vector<uint32_t> part_off;    // segs.size() + 1 entries
};

// check 3 (n_groups > 2^28, before anything is allocated), then the plan.  The group indices have passed locate_check_groups; count < 2^32.
inline int32_t locate_plan(const uint64_t* group_indices, size_t count, size_t n_groups, LocatePlan* plan) {
    *plan = LocatePlan();
    if (n_groups > LOCATE_MAX_GROUPS) return KZG_ERR_TOO_LARGE;
    plan->count = count; plan->n_groups = n_groups;
    plan->offsets.assign(n_groups + 1, 0);
    for (size_t i = 0; i < count; ++i) ++plan->offsets[group_indices[i] + 1];
    for (size_t g = 0; g < n_groups; ++g) plan->offsets[g + 1] += plan->offsets[g];
    plan->perm.resize(count);
    {
        std::vector<uint32_t> next(plan->offsets.begin(), plan->offsets.end() - 1);
        for (size_t i = 0; i < count; ++i) plan->perm[next[group_indices[i]]++] = (uint32_t)i;
    }
    plan->seg_of.resize(count);
    plan->seg_off.push_back(0);
    plan->part_off.push_back(0);
    for (size_t g = 0; g < n_groups; ++g) {
        const uint32_t a = plan->offsets[g], b = plan->offsets[g + 1];
        if (a == b) continue;
        const uint32_t j = (uint32_t)plan->segs.size();
        plan->segs.push_back((uint32_t)g);
        plan->seg_off.push_back(b);
        plan->part_off.push_back(plan->part_off.back() + ((b - 1) / LOCATE_WAVE - a / LOCATE_WAVE + 1));
        for (uint32_t s = a; s < b; ++s) plan->seg_of[s] = j;
    }
    return KZG_OK;
}

// The plan over a SUBSET of the items (the second level of kzg_retrieve_blobs_bytes_tolerant: the items of the bad blobs only).  Chosen item
// j is items[j] (an item of the call, any order, none twice) in group groups[j] < n_groups.  The plan has n_sel lanes -- count, offsets, segments
// and partial slots are those of locate_plan over the n_sel group indices -- and perm names the ITEMS, so the kernels, which read values, weights
// and points through perm, touch the chosen items only.  n_sel = 0 gives a plan without segments: nothing to launch.
inline int32_t locate_subset_plan(const uint32_t* items, const uint64_t* groups, size_t n_sel, size_t n_groups, LocatePlan* plan) {
    const int32_t rc = locate_plan(groups, n_sel, n_groups, plan);
    if (rc != KZG_OK) return rc;
    for (uint32_t& p : plan->perm) p = items[p];
    return KZG_OK;
}

// ceil(log2 n) for n >= 1
inline unsigned locate_log2_ceil(size_t n) {
    unsigned k = 0;
    while (((size_t)1 << k) < n) ++k;
    return k;
}
// the contract of locate_search: at most this many predicate calls for `bad` bad groups among n_groups
inline size_t locate_max_checks(size_t n_groups, size_t bad) { return 1 + 2 * bad * locate_log2_ceil(n_groups ? n_groups : 1); }

// The search.  leaves[g] is the pair (lhs, rhs) of group g's own equation; `holds(lhs, rhs)` says whether the equation of a SUM of such
// pairs holds.  Ops supplies the group law on the pair's components: P zero(), P add(P, P), P sub(P, P).
//   1. prefix sums of the leaves in group order: the pair of any range [a, b) is prefix[b] - prefix[a];
//   2. the root [0, n_groups) is tested;
//   3. a range that holds marks all its groups good.  That is sound only statistically: two bad groups inside one range could cancel.
//      With weights from a transcript over all inputs (kzg_compute_multiproof_r_powers) a cancellation is a non-trivial linear relation
//      between independent challenges: probability about (number of ranges) / r, negligible.  Weights the caller makes up give no such
//      guarantee;
//   4. a failing range of one group marks it bad;
//   5. otherwise the range is halved and the LEFT half tested; if it holds, the right half fails without a test.
// Every failing range costs at most two calls (its left half, and its right half when the left failed too), and the failing ranges are
// the ancestors of the bad leaves in a tree of depth ceil(log2 n_groups): at most 1 + 2 b ceil(log2 n_groups) calls for b bad groups.
// out_ok: n_groups bytes, 1 = good.  Returns the number of calls; *out_bad = the number of bad groups.  n_groups = 0: no call.
template <class P, class Ops, class Holds>
size_t locate_search(const P* lhs, const P* rhs, size_t n_groups, const Ops& ops, const Holds& holds, uint8_t* out_ok, size_t* out_bad) {
    size_t calls = 0, bad = 0;
    if (out_bad) *out_bad = 0;
    if (n_groups == 0) return 0;
    std::vector<P> pl(n_groups + 1), pr(n_groups + 1);
    pl[0] = ops.zero(); pr[0] = ops.zero();
    for (size_t g = 0; g < n_groups; ++g) { pl[g + 1] = ops.add(pl[g], lhs[g]); pr[g + 1] = ops.add(pr[g], rhs[g]); }
    auto range_holds = [&](size_t a, size_t b) {
        ++calls;
        return (bool)holds(ops.sub(pl[b], pl[a]), ops.sub(pr[b], pr[a]));
    };
    struct Todo { size_t a, b; bool fails; };                // fails: known without a test
    std::vector<Todo> stack;
    stack.push_back(Todo{0, n_groups, false});
    while (!stack.empty()) {
        const Todo t = stack.back();
        stack.pop_back();
        if (!t.fails && range_holds(t.a, t.b)) {
            for (size_t g = t.a; g < t.b; ++g) out_ok[g] = 1;
            continue;
        }
        if (t.b - t.a == 1) { out_ok[t.a] = 0; ++bad; continue; }
        const size_t mid = t.a + (t.b - t.a) / 2;
        if (range_holds(t.a, mid)) {
            for (size_t g = t.a; g < mid; ++g) out_ok[g] = 1;
            stack.push_back(Todo{mid, t.b, true});
        } else {
            stack.push_back(Todo{mid, t.b, false});
            stack.push_back(Todo{t.a, mid, true});
        }
    }
    if (out_bad) *out_bad = bad;
    return calls;
}

}  // namespace kzg
