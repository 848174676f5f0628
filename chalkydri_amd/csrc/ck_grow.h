// The buffers of the on-demand workspaces (JPEG decode, raw staging, preview, exposure, tri-class threshold, calibration, coloured pieces; one JPEG workspace per slot
// of a JPEG ingest ring): each owns its memory, grows when a call needs more and releases it when its workspace is deleted.  DESIGN.md §4g.
#ifndef CK_GROW_H
#define CK_GROW_H

#include <new>

#include "ck_internal.h"

// reserve(): at least `need` bytes.  A buffer that is large enough stays; otherwise it is freed and allocated again (its contents
// are never needed across a growth), `need` bytes exactly or with a quarter of headroom, so a stream of slowly growing calls
// does not reallocate every time.
template <typename T>
struct ck_dev_buf { // device memory through ck_malloc_dev: CK_POISON fill and guard pages apply
    T *p = nullptr;
    size_t cap = 0; // bytes
    ck_dev_buf() = default;
    ck_dev_buf(const ck_dev_buf &) = delete;
    ck_dev_buf &operator=(const ck_dev_buf &) = delete;
    ~ck_dev_buf() { (void)ck_free_dev(p); }
    operator T *() const { return p; }
    int reserve(size_t need, bool exact = false) { // CK_OK / CK_ENOMEM / CK_EDEVICE (ck_err_text set)
        if (need <= cap) return CK_OK;
        (void)ck_free_dev(p);
        p = nullptr; cap = 0;
        const size_t want = exact ? need : need + need / 4;
        CK_HIP_ALLOC(ck_malloc_dev(&p, want));
        cap = want;
        return CK_OK;
    }
};

// reserve() for `bytes + pad` and the copy of `bytes` of host memory up on `stream`; `pad` is what a kernel may read past the end
template <typename T>
static inline int ck_upload(ck_dev_buf<T> &b, const void *src, size_t bytes, hipStream_t stream, size_t pad = 0) {
    const int rc = b.reserve(bytes + pad);
    if (rc != CK_OK) return rc;
    if (bytes) CK_HIP(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, stream));
    return CK_OK;
}

template <typename T>
struct ck_pinned_buf { // pinned host memory
    T *p = nullptr;
    size_t cap = 0; // bytes
    ck_pinned_buf() = default;
    ck_pinned_buf(const ck_pinned_buf &) = delete;
    ck_pinned_buf &operator=(const ck_pinned_buf &) = delete;
    ~ck_pinned_buf() { if (p) (void)hipHostFree(p); }
    operator T *() const { return p; }
    int reserve(size_t need, bool exact = false) { // CK_OK / CK_ENOMEM
        if (need <= cap) return CK_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        const size_t want = exact ? need : need + need / 4;
        if (hipHostMalloc(reinterpret_cast<void **>(&p), want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            return CK_ENOMEM;
        }
        cap = want;
        return CK_OK;
    }
};

// A handle's workspace of one on-demand feature (`slot` = ck_handle::jpeg, raw, preview, exposure, tri_otsu or calib): created by the first call that
// needs it, deleted by ck_destroy.  nullptr: out of memory.
template <typename W>
static inline W *ck_workspace(W *&slot) {
    if (!slot) slot = new (std::nothrow) W();
    return slot;
}

#endif
