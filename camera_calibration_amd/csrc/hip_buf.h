// Owning, sized handles of device memory (DevBuf) and pinned host memory (PinnedBuf), and the error macros of the host code.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/cba.h"

namespace cba {

void set_error(const std::string& msg);
#define CBA_HIP(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      ::cba::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                     \
      return CBA_ERR_HIP;                                                                      \
    }                                                                                          \
  } while (0)
#define CBA_TRY(expr) do { int _rc = (expr); if (_rc != CBA_OK) return _rc; } while (0)

// elements [offset, offset + n) lie inside a buffer of `size` elements (no sum that could wrap)
constexpr bool span_fits(size_t size, size_t offset, size_t n) { return offset <= size && n <= size - offset; }
static_assert(span_fits(8, 8, 0) && span_fits(0, 0, 0) && !span_fits(8, 9, 0), "empty span at the end / past the end");
static_assert(span_fits(8, 5, 3) && !span_fits(8, 5, 4) && span_fits(8, 0, 8) && !span_fits(8, 0, 9), "offset + n exactly size / one past");
static_assert(!span_fits(8, 5, SIZE_MAX - 2) && !span_fits(SIZE_MAX, SIZE_MAX, 1) && !span_fits(8, SIZE_MAX, 2), "offset + n wraps");
inline int span_error(const char* op, size_t size, size_t offset, size_t n) {
  set_error(std::string("HipBuf::") + op + ": " + std::to_string(n) + " elements at offset " + std::to_string(offset) +
            " do not fit a buffer of " + std::to_string(size));
  return CBA_ERR_STATE;
}

// Host only, move-only.  alloc(n) first releases what the handle holds, then allocates (n = 0 allocates one element and reports
// size() 0); on failure the handle stays empty and the error is set as by CBA_HIP.  Every transfer, fill and clear counts in elements
// of T and is refused (CBA_ERR_STATE, no HIP call) unless it lies inside size(); n = 0 issues no HIP call.  `offset` is always this
// buffer's; the *_async forms take the stream after the length.  The read-only conversion keeps launch sites as they are (p->Dblk).
template <typename T, bool kPinned>
class HipBuf {
 public:
  using value_type = T;
  HipBuf() = default;
  HipBuf(HipBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  HipBuf& operator=(HipBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
    return *this;
  }
  ~HipBuf() { reset(); }
  int alloc(size_t n) {
    reset();
    void* q = nullptr;
    if (kPinned) CBA_HIP(hipHostMalloc(&q, (n ? n : 1) * sizeof(T)));
    else CBA_HIP(hipMalloc(&q, (n ? n : 1) * sizeof(T)));
    p_ = static_cast<T*>(q); n_ = n;
    return CBA_OK;
  }
  void reset() {
    if (p_) { if (kPinned) hipHostFree(p_); else hipFree(p_); }
    p_ = nullptr; n_ = 0;
  }
  size_t size() const { return n_; }
  operator T*() const { return p_; }

  int reserve(size_t n) { return p_ && n <= n_ ? CBA_OK : alloc(n); }      // grows only; the contents are lost when it grows
  int alloc_zero(size_t n) { CBA_TRY(alloc(n)); return zero(); }
  int assign(const T* host, size_t n) { CBA_TRY(alloc(n)); return upload(host, n); }
  int assign(const std::vector<T>& v) { return assign(v.data(), v.size()); }

  int upload(const T* host, size_t n, size_t offset = 0) { return to_device("upload", host, n, offset, nullptr); }
  int upload_async(const T* host, size_t n, hipStream_t s, size_t offset = 0) { return to_device("upload_async", host, n, offset, &s); }
  int upload_async(const HipBuf<T, true>& src, size_t n, hipStream_t s, size_t offset = 0, size_t src_offset = 0) {
    CBA_TRY(src.fits("upload_async (pinned side)", src_offset, n));
    return to_device("upload_async", src.p_ + src_offset, n, offset, &s);
  }
  int download(T* host, size_t n, size_t offset = 0) const { return to_host("download", host, n, offset, nullptr); }
  int download_optional(T* host_or_null, size_t n, size_t offset = 0) const { return host_or_null ? download(host_or_null, n, offset) : CBA_OK; }
  int download_async(T* host, size_t n, hipStream_t s, size_t offset = 0) const { return to_host("download_async", host, n, offset, &s); }
  int download_async(HipBuf<T, true>& dst, size_t n, hipStream_t s, size_t offset = 0, size_t dst_offset = 0) const {
    CBA_TRY(dst.fits("download_async (pinned side)", dst_offset, n));
    return to_host("download_async", dst.p_ + dst_offset, n, offset, &s);
  }
  int download_sync(T* host, size_t n, hipStream_t s, size_t offset = 0) const {      // download_async, then a wait for the stream
    CBA_TRY(download_async(host, n, s, offset));
    CBA_HIP(hipStreamSynchronize(s));
    return CBA_OK;
  }
  int copy_from_async(const HipBuf<T, false>& src, size_t n, size_t dst_offset, size_t src_offset, hipStream_t s) {
    CBA_TRY(fits("copy_from_async", dst_offset, n)); CBA_TRY(src.fits("copy_from_async (source)", src_offset, n));
    return copy(p_ + dst_offset, src.p_ + src_offset, n, hipMemcpyDeviceToDevice, &s);
  }
  int fill_bytes(int value, size_t n, size_t offset = 0) { return fill("fill_bytes", value, n, offset, nullptr); }
  int fill_bytes_async(int value, size_t n, hipStream_t s, size_t offset = 0) { return fill("fill_bytes_async", value, n, offset, &s); }
  int zero() { return fill("zero", 0, n_, 0, nullptr); }
  int zero(size_t n, size_t offset = 0) { return fill("zero", 0, n, offset, nullptr); }
  int zero_async(hipStream_t s) { return fill("zero_async", 0, n_, 0, &s); }
  int zero_async(size_t n, hipStream_t s, size_t offset = 0) { return fill("zero_async", 0, n, offset, &s); }

 private:
  template <typename, bool> friend class HipBuf;
  int fits(const char* op, size_t offset, size_t n) const { return span_fits(n_, offset, n) ? CBA_OK : span_error(op, n_, offset, n); }
  // s: null = the blocking call
  static int copy(T* dst, const T* src, size_t n, hipMemcpyKind kind, const hipStream_t* s) {
    if (!n) return CBA_OK;
    if (s) CBA_HIP(hipMemcpyAsync(dst, src, n * sizeof(T), kind, *s));
    else CBA_HIP(hipMemcpy(dst, src, n * sizeof(T), kind));
    return CBA_OK;
  }
  int to_device(const char* op, const T* host, size_t n, size_t offset, const hipStream_t* s) {
    static_assert(!kPinned, "transfers are operations of the device buffer");
    CBA_TRY(fits(op, offset, n));
    return copy(p_ + offset, host, n, hipMemcpyHostToDevice, s);
  }
  int to_host(const char* op, T* host, size_t n, size_t offset, const hipStream_t* s) const {
    static_assert(!kPinned, "transfers are operations of the device buffer");
    CBA_TRY(fits(op, offset, n));
    return copy(host, p_ + offset, n, hipMemcpyDeviceToHost, s);
  }
  int fill(const char* op, int value, size_t n, size_t offset, const hipStream_t* s) {
    static_assert(!kPinned, "fills are operations of the device buffer");
    CBA_TRY(fits(op, offset, n));
    if (!n) return CBA_OK;
    if (s) CBA_HIP(hipMemsetAsync(p_ + offset, value, n * sizeof(T), *s));
    else CBA_HIP(hipMemset(p_ + offset, value, n * sizeof(T)));
    return CBA_OK;
  }

  T* p_ = nullptr;
  size_t n_ = 0;
};
template <typename T> using DevBuf = HipBuf<T, false>;
template <typename T> using PinnedBuf = HipBuf<T, true>;

}  // namespace cba
