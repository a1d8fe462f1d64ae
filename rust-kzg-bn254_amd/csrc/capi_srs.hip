// capi_srs.hip — the kzg_srs_* surface of the C-ABI: upload / generation / decompression of an SRS, the packed-SRS file, Lagrange bases
// and their cache, the FK20 multi-proof tables and proofs, the encoder (cosets of values with their proofs).
#include "engine.h"
#include "host_sha256.h"

#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

using namespace kzg;

namespace kzg {
// off_curve != nullptr: the points are also validated on the device (y^2 == x^3 + 3 or identity); *off_curve = 1 if one fails
int32_t upload_points(kzg_ctx* ctx, const uint64_t* xy, size_t n, uint4* d_out, DeviceBuffer& staging, uint32_t* off_curve) {
    KZG_HIP_TRY(ctx, staging.reserve(n * 64 + 64));
    KZG_HIP_TRY(ctx, hipMemcpyAsync(staging.p, xy, n * 64, hipMemcpyHostToDevice, ctx->stream));
    uint32_t* d_flag = nullptr;
    if (off_curve) {
        d_flag = reinterpret_cast<uint32_t*>(static_cast<char*>(staging.p) + n * 64);
        KZG_HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, 4, ctx->stream));
    }
    int32_t rc = points_wire_to_device(ctx, staging.as<uint4>(), d_out, n, d_flag);
    if (rc != KZG_OK) return rc;
    if (off_curve) KZG_HIP_TRY(ctx, hipMemcpyAsync(off_curve, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    KZG_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KZG_OK;
}
}  // namespace kzg

namespace {
int32_t srs_upload_impl(kzg_ctx* ctx, const uint64_t* g1_xy_mont, size_t n_points, kzg_srs** out, bool tables) {
    if (!ctx || !out || (!g1_xy_mont && n_points)) return KZG_ERR_INVALID_ARG;
    *out = nullptr;
    if (n_points > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    kzg_srs* s = new (std::nothrow) kzg_srs();
    if (!s) return KZG_ERR_INVALID_ARG;
    s->ctx = ctx;
    s->n = n_points;
    if (n_points) {
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->d_points), n_points * 64);
        if (e != hipSuccess) { delete s; return set_error(ctx, e, "hipMalloc(srs)"); }
        int32_t rc = upload_points(ctx, g1_xy_mont, n_points, s->d_points, ctx->msm.bases_wire);
        if (rc == KZG_OK && tables) rc = srs_precompute(ctx, s);
        if (rc != KZG_OK) { (void)hipFree(s->d_points); delete s; return rc; }
    }
    *out = s;
    return KZG_OK;
}

int32_t srs_load_compressed(kzg_ctx* ctx, const uint8_t* bytes, size_t n_points, kzg_srs** out, uint64_t* bad_index, bool ark_le) {
    if (!ctx || !out || (n_points && !bytes)) return KZG_ERR_INVALID_ARG;
    *out = nullptr;
    if (n_points > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    kzg_srs* s = new (std::nothrow) kzg_srs();
    if (!s) return KZG_ERR_INVALID_ARG;
    s->ctx = ctx;
    s->n = n_points;
    if (n_points) {
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->d_points), n_points * 64);
        if (e != hipSuccess) { delete s; return set_error(ctx, e, "hipMalloc(srs)"); }
        uint32_t kind = 0, idx = 0;
        int32_t rc = srs_decompress(ctx, bytes, n_points, s->d_points, &kind, &idx, ark_le);
        if (rc == KZG_OK && kind != 0) {
            if (bad_index) *bad_index = idx;
            rc = kind == 1 ? KZG_ERR_DESERIALIZE : KZG_ERR_NOT_ON_CURVE;
        }
        if (rc == KZG_OK) rc = srs_precompute(ctx, s);
        if (rc != KZG_OK) { (void)hipFree(s->d_points); delete s; return rc; }
    }
    *out = s;
    return KZG_OK;
}

// ---- packed SRS file: the decoded points as they cross the C-ABI (64 B each), so that a restart skips the decoding of the ceremony file ----
// layout: "KZGSRS1\0" | u64 n | u64 0 | SHA-256 of the payload (32 B) | payload = n x 64 B (x || y Montgomery words, identity = zeros), little-endian
const char PACKED_MAGIC[8] = {'K', 'Z', 'G', 'S', 'R', 'S', '1', 0};
constexpr size_t PACKED_HEADER = 8 + 8 + 8 + 32;
void sha256_of(const uint8_t* data, size_t len, uint8_t out[32]) {
    kzg_host::Sha256 sh;
    kzg_host::sha256_init(sh);
    kzg_host::sha256_update(sh, data, len);
    kzg_host::sha256_final(sh, out);
}

// Lagrange basis of the first n points as an SRS of its own (device resident, with its window tables); len < n: only the points
// [lo, lo + len) of it are kept (a rank's shard of the basis, kzg_srs_lagrange_shard)
int32_t build_lagrange(kzg_ctx* ctx, const kzg_srs* srs, size_t n, kzg_srs** out, size_t lo = 0, size_t len = (size_t)-1) {
    if (n == 0 || (n & (n - 1)) != 0) return KZG_ERR_NOT_POWER_OF_TWO;             // kzg.rs:265-269
    if (n > ((size_t)1 << 28)) return KZG_ERR_DOMAIN;                               // kzg.rs:275-278
    if (n > srs->n) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    if (len == (size_t)-1) len = n;
    kzg_srs* s = new (std::nothrow) kzg_srs();
    if (!s) return KZG_ERR_INVALID_ARG;
    s->ctx = ctx;
    s->n = len;
    s->lagrange_of = n;
    uint4* full = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&full), n * 64);
    if (e != hipSuccess) { delete s; return set_error(ctx, e, "hipMalloc(lagrange srs)"); }
    int32_t rc = g1_ifft_device(ctx, srs, n, full, false);
    if (rc == KZG_OK) { hipError_t e2 = hipStreamSynchronize(ctx->stream); if (e2 != hipSuccess) rc = set_error(ctx, e2, "g1_ifft"); }
    if (rc == KZG_OK && len != n) {                                                 // keep the slice only
        uint4* part = nullptr;
        if (len) {
            e = hipMalloc(reinterpret_cast<void**>(&part), len * 64);
            if (e == hipSuccess) e = hipMemcpy(part, full + 4 * lo, len * 64, hipMemcpyDeviceToDevice);
            if (e != hipSuccess) { if (part) (void)hipFree(part); part = nullptr; rc = set_error(ctx, e, "lagrange shard"); }
        }
        (void)hipFree(full);
        full = part;
    }
    s->d_points = full;
    if (rc == KZG_OK && len) rc = srs_precompute(ctx, s);
    if (rc != KZG_OK) { if (s->d_points) (void)hipFree(s->d_points); delete s; return rc; }
    *out = s;
    return KZG_OK;
}

// ---- FK20 multi-proofs (multiproof.hip) ---------------------------------------------------------------------------------------
int32_t multiproof_check(kzg_ctx* ctx, const kzg_srs* srs, size_t n, size_t chunk_len) {
    if (!ctx || !srs || srs->ctx != ctx || srs->lagrange_of != 0) return KZG_ERR_INVALID_ARG;
    if (n == 0 || (n & (n - 1)) != 0) return KZG_ERR_NOT_POWER_OF_TWO;
    if (n == 1 || chunk_len == 0 || (chunk_len & (chunk_len - 1)) != 0 || chunk_len > n / 2) return KZG_ERR_INVALID_ARG;
    if (n > ((size_t)1 << 24)) return KZG_ERR_DOMAIN;
    if (n > srs->n) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    return KZG_OK;
}
}  // namespace

extern "C" {

int32_t kzg_srs_upload(kzg_ctx* ctx, const uint64_t* g1_xy_mont, size_t n_points, kzg_srs** out) {
    return srs_upload_impl(ctx, g1_xy_mont, n_points, out, true);
}

int32_t kzg_srs_generate(kzg_ctx* ctx, const uint64_t tau_mont[4], uint64_t first_power, size_t n_points, kzg_srs** out) {
    if (!ctx || !out || !tau_mont) return KZG_ERR_INVALID_ARG;
    *out = nullptr;
    if (n_points > ((size_t)1 << 28)) return KZG_ERR_TOO_LARGE;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    kzg_srs* s = new (std::nothrow) kzg_srs();
    if (!s) return KZG_ERR_INVALID_ARG;
    s->ctx = ctx;
    s->n = n_points;
    if (n_points) {
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->d_points), n_points * 64);
        if (e != hipSuccess) { delete s; return set_error(ctx, e, "hipMalloc(srs)"); }
        int32_t rc = srs_generate(ctx, tau_mont, first_power, n_points, s->d_points);
        if (rc == KZG_OK) rc = srs_precompute(ctx, s);
        if (rc != KZG_OK) { (void)hipFree(s->d_points); delete s; return rc; }
    }
    *out = s;
    return KZG_OK;
}

int32_t kzg_srs_load_compressed_be(kzg_ctx* ctx, const uint8_t* bytes, size_t n_points, kzg_srs** out, uint64_t* bad_index) {
    return srs_load_compressed(ctx, bytes, n_points, out, bad_index, false);
}
int32_t kzg_srs_load_compressed_ark_le(kzg_ctx* ctx, const uint8_t* bytes, size_t n_points, kzg_srs** out, uint64_t* bad_index) {
    return srs_load_compressed(ctx, bytes, n_points, out, bad_index, true);
}

int32_t kzg_srs_save_packed(kzg_ctx* ctx, const kzg_srs* srs, const char* path) {
    if (!ctx || !srs || srs->ctx != ctx || !path) return KZG_ERR_INVALID_ARG;
    std::vector<uint64_t> pts(srs->n * 8 + 1);
    if (srs->n) { const int32_t rc = kzg_srs_download(ctx, srs, 0, srs->n, pts.data()); if (rc != KZG_OK) return rc; }
    uint8_t head[PACKED_HEADER] = {0};
    memcpy(head, PACKED_MAGIC, 8);
    const uint64_t n64 = (uint64_t)srs->n;
    memcpy(head + 8, &n64, 8);
    sha256_of(reinterpret_cast<const uint8_t*>(pts.data()), srs->n * 64, head + 24);
    FILE* f = fopen(path, "wb");
    if (!f) { std::lock_guard<std::mutex> lk(ctx->mu); ctx->last_error = std::string("cannot create ") + path; return KZG_ERR_IO; }
    const bool ok = fwrite(head, 1, sizeof head, f) == sizeof head && (srs->n == 0 || fwrite(pts.data(), 64, srs->n, f) == srs->n);
    const bool closed = fclose(f) == 0;
    if (!ok || !closed) { std::lock_guard<std::mutex> lk(ctx->mu); ctx->last_error = std::string("short write to ") + path; return KZG_ERR_IO; }
    return KZG_OK;
}

int32_t kzg_srs_load_packed(kzg_ctx* ctx, const char* path, size_t points_to_load, kzg_srs** out) {
    if (!ctx || !path || !out) return KZG_ERR_INVALID_ARG;
    *out = nullptr;
    FILE* f = fopen(path, "rb");
    if (!f) { std::lock_guard<std::mutex> lk(ctx->mu); ctx->last_error = std::string("cannot open ") + path; return KZG_ERR_IO; }
    uint8_t head[PACKED_HEADER];
    uint64_t n64 = 0;
    std::vector<uint64_t> pts;
    int32_t rc = KZG_OK;
    if (fread(head, 1, sizeof head, f) != sizeof head || memcmp(head, PACKED_MAGIC, 8) != 0) rc = KZG_ERR_DESERIALIZE;
    if (rc == KZG_OK) {
        memcpy(&n64, head + 8, 8);
        if (n64 > ((uint64_t)1 << 28)) rc = KZG_ERR_TOO_LARGE;
    }
    if (rc == KZG_OK) {                                            // the header's count is believed only if the file has exactly that many bytes
        const long here = ftell(f);
        long size = -1;
        if (here >= 0 && fseek(f, 0, SEEK_END) == 0) { size = ftell(f); if (fseek(f, here, SEEK_SET) != 0) size = -1; }
        if (size < 0 || (uint64_t)size != (uint64_t)PACKED_HEADER + n64 * 64) rc = KZG_ERR_DESERIALIZE;   // truncated, or bytes behind the payload
    }
    if (rc == KZG_OK) {
        try { pts.resize((size_t)n64 * 8 + 1); } catch (const std::bad_alloc&) { rc = KZG_ERR_TOO_LARGE; }
        if (rc == KZG_OK && n64 && fread(pts.data(), 64, (size_t)n64, f) != (size_t)n64) rc = KZG_ERR_DESERIALIZE;
    }
    fclose(f);
    if (rc == KZG_OK) {
        uint8_t dig[32];
        sha256_of(reinterpret_cast<const uint8_t*>(pts.data()), (size_t)n64 * 64, dig);
        if (memcmp(dig, head + 24, 32) != 0) rc = KZG_ERR_DESERIALIZE;
    }
    if (rc != KZG_OK) { std::lock_guard<std::mutex> lk(ctx->mu); ctx->last_error = std::string(path) + ": not a packed SRS file of this library, or damaged"; return rc; }
    const size_t n = points_to_load ? points_to_load : (size_t)n64;
    if (n > (size_t)n64) return KZG_ERR_SRS_LENGTH;               // more points asked for than the file holds
    // the points are validated on the device while they are converted (y^2 = x^3 + 3 or the identity): a file from elsewhere cannot smuggle in garbage
    kzg_srs* s = nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
        s = new (std::nothrow) kzg_srs();
        if (!s) return KZG_ERR_INVALID_ARG;
        s->ctx = ctx;
        s->n = n;
        if (n) {
            hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->d_points), n * 64);
            if (e != hipSuccess) { delete s; return set_error(ctx, e, "hipMalloc(srs)"); }
            uint32_t off_curve = 0;
            rc = upload_points(ctx, pts.data(), n, s->d_points, ctx->msm.bases_wire, &off_curve);
            if (rc == KZG_OK && off_curve) rc = KZG_ERR_NOT_ON_CURVE;
            if (rc == KZG_OK) rc = srs_precompute(ctx, s);
            if (rc != KZG_OK) { (void)hipFree(s->d_points); delete s; return rc; }
        }
    }
    *out = s;
    return KZG_OK;
}

int32_t kzg_srs_download(kzg_ctx* ctx, const kzg_srs* srs, size_t offset, size_t n, uint64_t* out_xy_mont) {
    if (!ctx || !srs || srs->ctx != ctx || (n && !out_xy_mont)) return KZG_ERR_INVALID_ARG;
    if (offset > srs->n || n > srs->n - offset) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return srs_download(ctx, srs->d_points + 4 * offset, n, out_xy_mont);
}

void kzg_srs_free(kzg_srs* srs) {
    if (!srs) return;
    for (auto& kv : srs->lagrange) kzg_srs_free(kv.second);
    srs->lagrange.clear();
    if (srs->d_points) { (void)hipSetDevice(srs->ctx->device); (void)hipFree(srs->d_points); }
    if (srs->d_small) { (void)hipSetDevice(srs->ctx->device); (void)hipFree(srs->d_small); }
    if (srs->d_bits) { (void)hipSetDevice(srs->ctx->device); (void)hipFree(srs->d_bits); }
    if (srs->d_t3) { (void)hipSetDevice(srs->ctx->device); (void)hipFree(srs->d_t3); }
    if (!srs->multiproof.empty()) { (void)hipSetDevice(srs->ctx->device); multiproof_drop(srs); }
    delete srs;
}

size_t kzg_srs_len(const kzg_srs* srs) { return srs ? srs->n : 0; }
int32_t kzg_srs_has_bit_tables(kzg_srs* srs, int32_t build) {
    if (!srs) return 0;
    if (srs_bits(srs)) return 1;
    if (!build || !srs->ctx) return 0;
    std::lock_guard<std::mutex> lk(srs->ctx->mu);
    if (hipSetDevice(srs->ctx->device) != hipSuccess) return 0;
    (void)srs_build_bit_tables(srs->ctx, srs, true);
    return srs_bits(srs) ? 1 : 0;
}

int32_t kzg_srs_lagrange(kzg_ctx* ctx, const kzg_srs* srs, size_t n, kzg_srs** out) {
    if (!ctx || !srs || srs->ctx != ctx || !out) return KZG_ERR_INVALID_ARG;
    *out = nullptr;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return build_lagrange(ctx, srs, n, out);
}

int32_t kzg_srs_lagrange_shard(kzg_ctx* ctx, const kzg_srs* srs, size_t n, size_t lo, size_t len, kzg_srs** out) {
    if (!ctx || !srs || srs->ctx != ctx || !out) return KZG_ERR_INVALID_ARG;
    *out = nullptr;
    if (lo > n || len > n - lo) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return build_lagrange(ctx, srs, n, out, lo, len);
}

int32_t kzg_srs_slice(kzg_ctx* ctx, const kzg_srs* srs, size_t lo, size_t len, kzg_srs** out) {
    if (!ctx || !srs || srs->ctx->device != ctx->device || !out) return KZG_ERR_INVALID_ARG;
    *out = nullptr;
    if (lo > srs->n || len > srs->n - lo) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    kzg_srs* s = new (std::nothrow) kzg_srs();
    if (!s) return KZG_ERR_INVALID_ARG;
    s->ctx = ctx;
    s->n = len;
    s->lagrange_of = srs->lagrange_of;
    if (len) {
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->d_points), len * 64);
        if (e == hipSuccess) e = hipMemcpy(s->d_points, srs->d_points + 4 * lo, len * 64, hipMemcpyDeviceToDevice);   // table 0 of `srs` = its points
        if (e != hipSuccess) { if (s->d_points) (void)hipFree(s->d_points); delete s; return set_error(ctx, e, "kzg_srs_slice"); }
        int32_t rc = srs_precompute(ctx, s);
        if (rc != KZG_OK) { (void)hipFree(s->d_points); delete s; return rc; }
    }
    *out = s;
    return KZG_OK;
}

int32_t kzg_srs_cache_lagrange(kzg_ctx* ctx, kzg_srs* srs, size_t n) {
    if (!ctx || !srs || srs->ctx != ctx) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (srs_cached_lagrange(srs, n)) return KZG_OK;
    kzg_srs* l = nullptr;
    int32_t rc = build_lagrange(ctx, srs, n, &l);           // (under ctx->mu: one builder at a time; complete and synchronised on return)
    if (rc != KZG_OK) return rc;
    std::lock_guard<std::mutex> lazy(srs->lazy_mu);
    srs->lagrange[n] = l;
    return KZG_OK;
}

int32_t kzg_srs_drop_lagrange(kzg_ctx* ctx, kzg_srs* srs) {
    if (!ctx || !srs || srs->ctx != ctx) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    std::lock_guard<std::mutex> lazy(srs->lazy_mu);
    for (auto& kv : srs->lagrange) kzg_srs_free(kv.second);
    srs->lagrange.clear();
    return KZG_OK;
}

int32_t kzg_compute_multiproofs(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* poly_mont, size_t n, int32_t eval_form,
                                size_t chunk_len, uint64_t* out_xy_mont, uint8_t* out_is_infinity) {
    if (!poly_mont || !out_xy_mont || !out_is_infinity) return KZG_ERR_INVALID_ARG;
    int32_t rc = multiproof_check(ctx, srs, n, chunk_len);
    if (rc != KZG_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return multiproof_run(ctx, srs, poly_mont, n, eval_form != 0, chunk_len, out_xy_mont, out_is_infinity);
}

int32_t kzg_encode_cosets(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* poly_mont, size_t poly_len, int32_t eval_form, size_t n, size_t chunk_len,
                          uint64_t* out_ys_mont, uint64_t* out_proofs_xy_mont, uint8_t* out_is_infinity) {
    const bool bad_pointers = !ctx || !srs || !poly_mont || (!out_ys_mont && !out_proofs_xy_mont) || (out_proofs_xy_mont && !out_is_infinity);
    const bool bad_srs = !bad_pointers && (srs->ctx != ctx || srs->lagrange_of != 0);
    int32_t rc = encode_check(bad_pointers, bad_srs, poly_len, n, chunk_len, srs ? srs->n : 0);
    if (rc != KZG_OK) return rc;
    const EncodePlan plan = encode_plan(poly_len, n, chunk_len, out_ys_mont != nullptr, out_proofs_xy_mont != nullptr);
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return multiproof_encode(ctx, srs, poly_mont, eval_form != 0, plan, out_ys_mont, out_proofs_xy_mont, out_is_infinity);
}

int32_t kzg_encode_cosets_batch(kzg_ctx* ctx, kzg_srs* srs, const uint64_t* polys_mont, size_t count, size_t poly_len, int32_t eval_form, size_t n,
                                size_t chunk_len, uint64_t* out_ys_mont, uint64_t* out_proofs_xy_mont, uint8_t* out_is_infinity) {
    const bool bad_pointers = !ctx || !srs || !polys_mont || (!out_ys_mont && !out_proofs_xy_mont) || (out_proofs_xy_mont && !out_is_infinity);
    const bool bad_srs = !bad_pointers && (srs->ctx != ctx || srs->lagrange_of != 0);
    int32_t rc = encode_batch_check(bad_pointers, bad_srs, count, poly_len, n, chunk_len, srs ? srs->n : 0);
    if (rc != KZG_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const EncodeBatchPlan plan = encode_batch_plan(poly_len, n, chunk_len, count, out_ys_mont != nullptr, out_proofs_xy_mont != nullptr, ctx->encode_group_bytes);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return multiproof_encode_batch(ctx, srs, polys_mont, eval_form != 0, plan, out_ys_mont, out_proofs_xy_mont, out_is_infinity);
}

// ---- the encoder in serialized form: bytes in, bytes out (multiproof.hip encode_groups with an EncodeBytesIo) -----------------------------------
// the host checks of kzg_encode_cosets_batch_bytes in their order: rows 1 - 7 of kzg_encode_cosets_batch with this entry's pointers, then count x poly_len
static int32_t encode_bytes_check(kzg_ctx* ctx, kzg_srs* srs, const uint8_t* blobs_be, size_t count, size_t poly_len, size_t n, size_t chunk_len, bool no_output) {
    const bool bad_pointers = !ctx || !srs || !blobs_be || no_output;
    const bool bad_srs = !bad_pointers && (srs->ctx != ctx || srs->lagrange_of != 0);
    int32_t rc = encode_batch_check(bad_pointers, bad_srs, count, poly_len, n, chunk_len, srs ? srs->n : 0);
    if (rc != KZG_OK) return rc;
    if (count > ((size_t)1 << 28) / poly_len) return KZG_ERR_TOO_LARGE;                // the bad word holds (b poly_len + i) << 2
    return KZG_OK;
}
// under ctx->mu: slot 0 idle (the commitments run on the slots), the plan with the context's budget, the run, the status of a refused value
static int32_t encode_bytes_run(kzg_ctx* ctx, kzg_srs* srs, const char* who, size_t count, size_t poly_len, int32_t eval_form, size_t n, size_t chunk_len, EncodeBytesIo& io,
                                uint64_t* bad_index) {
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (slot0_refused(ctx)) return KZG_ERR_INVALID_ARG;
    const EncodeBatchPlan plan = encode_batch_plan(poly_len, n, chunk_len, count, io.ys_be != nullptr, io.proofs_be != nullptr, ctx->encode_group_bytes);
    uint32_t bad_word = 0xFFFFFFFFu;
    io.bad_word = &bad_word;
    const int32_t rc = multiproof_encode_batch_bytes(ctx, srs, eval_form != 0, plan, io);
    if (rc == KZG_ERR_DESERIALIZE) return coset_bytes_status(ctx, who, "value", bad_word, 1, bad_index);
    return rc;
}

int32_t kzg_encode_cosets_batch_bytes(kzg_ctx* ctx, kzg_srs* srs, const uint8_t* blobs_be, size_t count, size_t poly_len, int32_t eval_form, size_t n, size_t chunk_len,
                                      uint8_t* out_commitments_be, uint8_t* out_ys_be, uint8_t* out_proofs_be, uint64_t* bad_index) {
    int32_t rc = encode_bytes_check(ctx, srs, blobs_be, count, poly_len, n, chunk_len, !out_commitments_be && !out_ys_be && !out_proofs_be);
    if (rc != KZG_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    EncodeBytesIo io;
    io.blobs_be = blobs_be; io.ys_be = out_ys_be; io.proofs_be = out_proofs_be; io.commitments_be = out_commitments_be;
    return encode_bytes_run(ctx, srs, "kzg_encode_cosets_batch_bytes", count, poly_len, eval_form, n, chunk_len, io, bad_index);
}

int32_t kzg_disperse_blobs_bytes(kzg_ctx* ctx, kzg_srs* srs, const kzg_g2srs* g2_srs, const kzg_g2srs* g2_trailing, uint64_t trailing_first_power, uint64_t srs_order,
                                 const uint8_t* blobs_be, size_t count, size_t poly_len, size_t n, size_t chunk_len, uint64_t claimed_len, uint8_t* out_commitments_be,
                                 uint8_t* out_length_commitments_be, uint8_t* out_length_proofs_be, uint8_t* out_ys_be, uint8_t* out_proofs_be, uint64_t* bad_index) {
    // the header is one unit: its three outputs are required; the chunks stay optional
    const bool no_header = !g2_srs || !g2_trailing || !out_commitments_be || !out_length_commitments_be || !out_length_proofs_be;
    int32_t rc = encode_bytes_check(ctx, srs, blobs_be, count, poly_len, n, chunk_len, no_header);
    if (rc != KZG_OK) return rc;
    if (g2_srs->ctx->device != ctx->device || g2_trailing->ctx->device != ctx->device) return KZG_ERR_INVALID_ARG;
    // rows 3 onward of kzg_commit_with_length_proof_batch, the polynomial length being poly_len
    const auto pow2 = [](uint64_t v) { return v != 0 && (v & (v - 1)) == 0; };
    if (!pow2(srs_order) || !pow2(claimed_len)) return KZG_ERR_NOT_POWER_OF_TWO;
    if (poly_len > claimed_len || claimed_len > srs_order) return KZG_ERR_INVALID_ARG;
    if (srs_order - claimed_len < trailing_first_power) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    const uint64_t off = srs_order - claimed_len - trailing_first_power;
    if (off > g2_trailing->n || claimed_len > g2_trailing->n - off) return KZG_ERR_SRS_CAPACITY_EXCEEDED;
    if (poly_len > g2_srs->n) return KZG_ERR_POLY_LENGTH;                                  // (poly_len <= the G1 SRS: row 6 above)
    std::lock_guard<std::mutex> lk(ctx->mu);
    EncodeBytesIo io;
    io.blobs_be = blobs_be; io.ys_be = out_ys_be; io.proofs_be = out_proofs_be; io.commitments_be = out_commitments_be;
    io.g2_points[0] = g2_srs->d_points; io.g2_points[1] = g2_trailing->d_points + 8 * off;
    io.length_commitments_be = out_length_commitments_be; io.length_proofs_be = out_length_proofs_be;
    return encode_bytes_run(ctx, srs, "kzg_disperse_blobs_bytes", count, poly_len, 0, n, chunk_len, io, bad_index);
}

int32_t kzg_ctx_set_encode_group_bytes(kzg_ctx* ctx, size_t bytes) {
    if (!ctx) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->encode_group_bytes = bytes;
    return KZG_OK;
}

static void encode_info_transform(const G1fftPlan& p, kzg_encode_transform_info* t) {
    t->form = p.form == G1FFT_COPY ? KZG_ENCODE_FORM_COPY : p.form == G1FFT_RADIX2 ? KZG_ENCODE_FORM_RADIX2 : KZG_ENCODE_FORM_DIRECT;
    t->load = KZG_ENCODE_LOAD_IN_PLACE;
    t->pairs = 0;
    t->stages = 0;
    for (int i = 0; i < p.n_stages; ++i) {
        const G1fftStage& st = p.stage[i];
        if (st.K > 0) { ++t->stages; t->pairs = st.kind == G1S_DIRECT_PAIRS || st.kind == G1S_RADIX2_PAIRS; }
        else t->load = st.kind == G1S_GATHER ? KZG_ENCODE_LOAD_COPY : st.kind == G1S_GATHER_BITREV ? KZG_ENCODE_LOAD_BITREV
                     : st.kind == G1S_GATHER_PAD ? KZG_ENCODE_LOAD_PAD : KZG_ENCODE_LOAD_SPREAD;
    }
}

int32_t kzg_encode_cosets_batch_info(size_t poly_len, size_t n, size_t chunk_len, size_t count, int32_t values, int32_t proofs, size_t group_bytes,
                                     kzg_encode_batch_info* out) {
    int32_t rc = encode_batch_check(!out || (!values && !proofs), false, count, poly_len, n, chunk_len, SIZE_MAX);
    if (rc != KZG_OK) return rc;
    const EncodeBatchPlan bp = encode_batch_plan(poly_len, n, chunk_len, count, values != 0, proofs != 0, group_bytes);
    *out = kzg_encode_batch_info{};
    out->blobs_per_group = bp.group;
    out->groups = bp.n_groups;
    out->group_bytes = bp.group_bytes;
    out->batched = bp.batched ? 1 : 0;
    if (proofs) {
        // a group of one runs kzg_encode_cosets' own launches: its plans are those of one transform, which is what batch = 1 gives
        encode_info_transform(bp.ifft, &out->inverse);
        encode_info_transform(bp.fft.plan, &out->forward);
    }
    return KZG_OK;
}

int32_t kzg_srs_cache_multiproof(kzg_ctx* ctx, kzg_srs* srs, size_t n, size_t chunk_len) {
    int32_t rc = multiproof_check(ctx, srs, n, chunk_len);
    if (rc != KZG_OK) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint4* table = nullptr;
    return multiproof_cache(ctx, srs, n, chunk_len, &table);
}

int32_t kzg_srs_drop_multiproof(kzg_ctx* ctx, kzg_srs* srs) {
    if (!ctx || !srs || srs->ctx != ctx) return KZG_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    KZG_HIP_TRY(ctx, hipSetDevice(ctx->device));
    multiproof_drop(srs);
    return KZG_OK;
}

}  // extern "C"

namespace kzg {
int32_t srs_upload_plain(kzg_ctx* ctx, const uint64_t* g1_xy_mont, size_t n_points, kzg_srs** out) { return srs_upload_impl(ctx, g1_xy_mont, n_points, out, false); }
}  // namespace kzg

#if defined(KZG_DEVICE_BOUND_CHECK)
#include "field29.h"
KZG_BOUND_CHECK_EXPORTS(capi_srs)
#endif
