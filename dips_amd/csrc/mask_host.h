// mask_host.h -- what the entry points of mask_abi.hip share: the byte size
// of a packed frame, the region and overlap checks, and HostStaging, the one
// path by which a call's host pointers travel through the handle's staging
// buffers.  Internal to libdips_hip.so.
#pragma once

#include <initializer_list>
#include <string>

#include "series_host.h"

namespace dips_internal {

// bytes of one w x hgt frame of a packed mask
inline size_t mask_frame_bytes(uint32_t w, uint32_t hgt) { return (size_t)(4u * mask_words_per_row(w) * hgt); }

// The region of a mask product under the exported function's `name` (the
// labelling family words it differently: check_labelling in mask_abi.hip)
inline dips_status check_mask_region(dips_handle* h, const char* name, uint32_t roi_w, uint32_t roi_h) {
    if (roi_w == 0 || roi_h == 0)
        return fail(h, DIPS_ERR_INVALID, std::string(name) + ": roi_w and roi_h must not be 0");
    if ((uint64_t)roi_w * roi_h >= (1ull << 30))
        return fail(h, DIPS_ERR_INVALID, std::string(name) + ": the region must stay below 2^30 pixels");
    return DIPS_OK;
}

struct ByteRange {
    const void* p;
    size_t n;
};

// whether two byte ranges share a byte (a NULL or empty range shares none)
inline bool ranges_overlap(ByteRange a, ByteRange b) {
    const uintptr_t pa = (uintptr_t)a.p, pb = (uintptr_t)b.p;
    return a.p && b.p && a.n != 0 && b.n != 0 && pa < pb + b.n && pb < pa + a.n;
}

// whether an output shares a byte with an input or with another output
inline bool outputs_overlap(std::initializer_list<ByteRange> outs, std::initializer_list<ByteRange> ins) {
    for (const ByteRange* o = outs.begin(); o != outs.end(); ++o) {
        for (const ByteRange& i : ins)
            if (ranges_overlap(*o, i)) return true;
        for (const ByteRange* o2 = o + 1; o2 != outs.end(); ++o2)
            if (ranges_overlap(*o, *o2)) return true;
    }
    return false;
}

// The pointers of one call.  An entry point adds each input and output once
// (at most 8) -- its staging buffer of the handle, the pointer variable, the
// byte count and kIn, kOut or kInOut --, then calls begin(), its
// run_*_device function with those same variables, and finish().  A NULL
// pointer or no bytes: the piece is absent.
//   DIPS_FLAG_DEVICE_PTRS: the variables stay as they are; check_aligned4()
//   refuses a pointer off a 4-byte boundary (pieces added with kAnyAlign are
//   not looked at), upload() and finish() do nothing.
//   Host pointers (a synchronous call): upload() grows every buffer first --
//   growing synchronises, and a failed grow must leave nothing copied --, has
//   the pieces of a buffer packed in the order added, points the variables at
//   the device copies (NULL for an absent piece) and uploads the ins;
//   finish() downloads the outs and synchronises the stream.
class HostStaging {
public:
    enum : unsigned { kIn = 1u, kOut = 2u, kInOut = 3u, kAnyAlign = 4u };

    HostStaging(dips_handle* h, const char* name) : h_(h), name_(name) {}
    bool device() const { return (h_->p.flags & DIPS_FLAG_DEVICE_PTRS) != 0; }

    template <typename T>
    void add(dips_host::DevBuf& buf, T*& ptr, size_t bytes, unsigned flags) {
        size_t off = 0;  // behind the buffer's pieces so far
        for (int k = 0; k < n_; ++k)
            if (pieces_[k].buf == &buf) off = pieces_[k].off + pieces_[k].bytes;
        pieces_[n_++] = Piece{&buf, const_cast<void*>(static_cast<const void*>(ptr)), off, ptr ? bytes : 0u, flags, &ptr,
                              [](void* var, void* dev) { *static_cast<T**>(var) = static_cast<T*>(dev); }};
    }

    dips_status check_aligned4() {
        uintptr_t bits = 0;
        for (int i = 0; i < n_; ++i)
            if (!(pieces_[i].flags & kAnyAlign)) bits |= (uintptr_t)pieces_[i].host;
        if (device() && (bits & 3u) != 0)
            return fail(h_, DIPS_ERR_INVALID, std::string(name_) + ": the device pointers must be 4-byte aligned");
        return DIPS_OK;
    }

    dips_status upload() {
        if (device()) return DIPS_OK;
        // a buffer's last piece ends at the buffer's size; its earlier ones then find it grown
        for (int i = n_; i-- > 0;) DIPS_HIP(h_, pieces_[i].buf->ensure(pieces_[i].off + pieces_[i].bytes));
        for (int i = 0; i < n_; ++i) {
            const Piece& p = pieces_[i];
            p.set(p.var, dev(p));
            if (p.bytes && (p.flags & kIn))
                DIPS_HIP(h_, hipMemcpyAsync(dev(p), p.host, p.bytes, hipMemcpyHostToDevice, h_->stream));
        }
        return DIPS_OK;
    }

    dips_status begin() {
        DIPS_TRY(check_aligned4());
        return upload();
    }

    dips_status finish() {
        if (device()) return DIPS_OK;
        for (int i = 0; i < n_; ++i) {
            const Piece& p = pieces_[i];
            if (p.bytes && (p.flags & kOut))
                DIPS_HIP(h_, hipMemcpyAsync(p.host, dev(p), p.bytes, hipMemcpyDeviceToHost, h_->stream));
        }
        DIPS_HIP(h_, hipStreamSynchronize(h_->stream));
        return DIPS_OK;
    }

private:
    struct Piece {
        dips_host::DevBuf* buf;
        void* host;
        size_t off, bytes;  // within buf
        unsigned flags;
        void* var;                  // the caller's pointer variable
        void (*set)(void*, void*);  // points it at a device copy
    };
    static void* dev(const Piece& p) { return p.bytes ? p.buf->as<uint8_t>() + p.off : nullptr; }

    dips_handle* h_;
    const char* name_;
    Piece pieces_[8];
    int n_ = 0;
};

}  // namespace dips_internal
