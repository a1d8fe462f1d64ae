// byte_stager.h — how untrusted host bytes reach the device in the serialized-input decoders (g2decode.hip, cosetbytes.hip,
// headerbytes.hip).  Host code on the HIP runtime: only .hip units include it.
//
// The bytes go up in pieces of at most STAGE_CHUNK_BYTES through the two halves of slot 0's pinned MSM result buffer (msm_pinned_out):
// one half is filled by the host while the other is read by a copy in flight, so no pinned allocation grows with the input.  A decode
// kernel starts behind every launch_bytes staged, not behind the whole input.  The rules every user depends on:
//   - A half is written only after the copy that last read it has finished: copy() waits on the half's event before its memcpy.  ONE
//     stager owns the piece counter for a whole call, so consecutive pieces alternate halves whatever array they belong to; a callee
//     that stages more in the same call is handed the caller's stager (coset_bytes_enqueue) and never starts a second one.
//   - The pinned buffer belongs to the MSM driver: slot 0 is idle for the whole call (every caller holds ctx->mu), and whatever used the
//     buffer before has been synchronised with when the stager is initialised, so the first two pieces wait on nothing.
//   - When a function that used the stager returns an error, it drains the stream first: the halves are still being read.  On success
//     the copies are ordered on the stream in front of everything enqueued after them, and the halves are next written by an MSM's
//     reduction on this stream or by a later call's stager, behind a synchronisation.  The events go with the object.
//   - Bad words are set on the device (hipMemsetAsync), never copied from a stack variable; a read-back INTO a local is followed by a
//     synchronisation on every path.
#pragma once
#include "msm_limits.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace kzg {

constexpr size_t STAGE_CHUNK_BYTES = (size_t)1 << 20;               // bytes per staged piece
static_assert(2 * STAGE_CHUNK_BYTES <= (size_t)MSM_MAX_OUT * 128, "two pieces fit the pinned result buffer");

struct ByteStager {
    hipStream_t st = nullptr;
    char* pinned = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    size_t piece = 0;
    ByteStager() = default;
    ByteStager(const ByteStager&) = delete;
    ByteStager& operator=(const ByteStager&) = delete;
    ~ByteStager() { for (hipEvent_t v : ev) if (v) (void)hipEventDestroy(v); }
    hipError_t init(hipStream_t stream, void* pinned_buf) {
        st = stream;
        pinned = static_cast<char*>(pinned_buf);
        for (hipEvent_t& v : ev) { const hipError_t e = hipEventCreateWithFlags(&v, hipEventDisableTiming); if (e != hipSuccess) return e; }
        return hipSuccess;
    }
    // one piece: len <= STAGE_CHUNK_BYTES bytes of src -> d_dst, through the next half
    hipError_t copy(const uint8_t* src, size_t len, char* d_dst) {
        const size_t half = piece & 1;
        char* h = pinned + half * STAGE_CHUNK_BYTES;
        hipError_t e = piece >= 2 ? hipEventSynchronize(ev[half]) : hipSuccess;          // the copy that last read this half has finished
        if (e != hipSuccess) return e;
        memcpy(h, src, len);
        ++piece;
        e = hipMemcpyAsync(d_dst, h, len, hipMemcpyHostToDevice, st);
        return e == hipSuccess ? hipEventRecord(ev[half], st) : e;
    }
    // one array: bytes of src -> d_dst; launch(lo, hi) is called behind the copies of every launch_bytes bytes and at the end (byte offsets)
    template <class Launch>
    hipError_t push(const uint8_t* src, size_t bytes, char* d_dst, size_t launch_bytes, Launch&& launch) {
        size_t launched = 0;
        for (size_t lo = 0; lo < bytes; lo += STAGE_CHUNK_BYTES) {
            const size_t len = std::min(STAGE_CHUNK_BYTES, bytes - lo);
            hipError_t e = copy(src + lo, len, d_dst + lo);
            if (e != hipSuccess) return e;
            const size_t staged = lo + len;
            if (staged - launched >= launch_bytes || staged == bytes) {
                launch(launched, staged);
                e = hipGetLastError();
                if (e != hipSuccess) return e;
                launched = staged;
            }
        }
        return hipSuccess;
    }
};

}  // namespace kzg
