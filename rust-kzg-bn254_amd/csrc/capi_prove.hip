// capi_prove.hip — the C-ABI of the selected-coset prover (provecosets.hip): kzg_prove_cosets, kzg_coset_quotients and the pure query
// kzg_prove_cosets_info.  Every check runs on the host before any launch, in the order of the header's table (host_prove_cosets.h).
#include "engine.h"

namespace {
using namespace kzg;

// checks 3 .. 5, the plan, the lock and the run, shared by the two entries (checks 1 and 2 are the caller's flags)
int32_t prove_common(kzg_ctx* ctx, kzg_srs* srs, bool bad_pointers, bool bad_srs, const uint64_t* polys_mont, size_t count, size_t poly_len, int32_t eval_form,
                     size_t n, size_t chunk_len, const uint64_t* poly_indices, const uint64_t* coset_indices, size_t n_items, uint64_t* out_q, uint64_t* out_ys,
                     uint64_t* out_xy, uint8_t* out_inf, uint64_t* bad_index) {
    int32_t rc = prove_cosets_check_shape(bad_pointers, bad_srs, count, poly_len, n, chunk_len, srs ? srs->n : SIZE_MAX);
    if (rc != KZG_OK) return rc;
    rc = prove_cosets_check_items(poly_indices, coset_indices, n_items, count, n / chunk_len, bad_index);
    if (rc != KZG_OK) return rc;
    const bool quotients = out_q != nullptr || out_xy != nullptr;
    rc = prove_cosets_check_sizes(count, poly_len, chunk_len, n_items, out_q != nullptr);
    if (rc != KZG_OK) return rc;
    if (n_items == 0) return KZG_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (slot0_refused(ctx)) return KZG_ERR_INVALID_ARG;
    const ProveCosetsPlan plan = prove_cosets_plan(poly_len, n, chunk_len, n_items, out_ys != nullptr, quotients, ctx->encode_group_bytes);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return prove_cosets_run(ctx, srs, polys_mont, count, eval_form != 0, plan, poly_indices, coset_indices, out_q, out_ys, out_xy, out_inf);
}
}  // namespace

extern "C" {

int32_t kzg_prove_cosets(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* polys_mont, size_t count, size_t poly_len, int32_t eval_form, size_t n, size_t chunk_len,
                         const uint64_t* poly_indices, const uint64_t* coset_indices, size_t n_items, uint64_t* out_ys_mont, uint64_t* out_proofs_xy_mont,
                         uint8_t* out_is_infinity, uint64_t* bad_index) {
    const bool bad_pointers = !ctx || !srs || !polys_mont || !coset_indices || (!out_ys_mont && !out_proofs_xy_mont) || (out_proofs_xy_mont && !out_is_infinity);
    const bool bad_srs = !bad_pointers && (srs->ctx != ctx || srs->lagrange_of != 0);
    return prove_common(ctx, bad_pointers ? nullptr : srs, bad_pointers, bad_srs, polys_mont, count, poly_len, eval_form, n, chunk_len, poly_indices, coset_indices,
                        n_items, nullptr, out_ys_mont, out_proofs_xy_mont, out_is_infinity, bad_index);
}

int32_t kzg_coset_quotients(kzg_ctx* ctx, const uint64_t* polys_mont, size_t count, size_t poly_len, int32_t eval_form, size_t n, size_t chunk_len,
                            const uint64_t* poly_indices, const uint64_t* coset_indices, size_t n_items, uint64_t* out_q_mont, uint64_t* out_ys_mont,
                            uint64_t* bad_index) {
    const bool bad_pointers = !ctx || !polys_mont || !coset_indices || (!out_q_mont && !out_ys_mont);
    return prove_common(ctx, nullptr, bad_pointers, false, polys_mont, count, poly_len, eval_form, n, chunk_len, poly_indices, coset_indices, n_items, out_q_mont,
                        out_ys_mont, nullptr, nullptr, bad_index);
}

int32_t kzg_prove_cosets_info(size_t poly_len, size_t n, size_t chunk_len, size_t count, size_t n_items, int32_t values, int32_t proofs, size_t group_bytes,
                              kzg_prove_cosets_info_t* out) {
    int32_t rc = prove_cosets_check_shape(!out || (!values && !proofs), false, count, poly_len, n, chunk_len, SIZE_MAX);
    if (rc != KZG_OK) return rc;
    rc = prove_cosets_check_sizes(count, poly_len, chunk_len, n_items, false);
    if (rc != KZG_OK) return rc;
    const ProveCosetsPlan p = prove_cosets_plan(poly_len, n, chunk_len, n_items, values != 0, proofs != 0, group_bytes);
    *out = kzg_prove_cosets_info_t{};
    out->items_per_group = p.group;
    out->groups = p.n_groups;
    out->group_bytes = p.group_bytes;
    out->item_bytes = p.item_bytes;
    out->seg_len = p.S;
    out->segments = p.level[0].nseg;
    out->carry_levels = (uint32_t)p.carry_levels();
    out->launches = p.launches;
    out->msm_single = proofs && p.msm_single ? 1u : 0u;
    return KZG_OK;
}

}  // extern "C"

#if defined(KZG_DEVICE_BOUND_CHECK)
#include "field29.h"
KZG_BOUND_CHECK_EXPORTS(capi_prove)
#endif
