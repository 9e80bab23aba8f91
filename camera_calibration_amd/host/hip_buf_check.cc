// Check program of csrc/hip_buf.h (host HIP API only, no kernels): every refused transfer must leave the device untouched and name
// the operation and its three numbers.  `--no-device` runs the cases that make no HIP call.  Exit status 0 = all cases passed.
#include <cstdio>
#include <cstring>
#include <utility>

#include "../csrc/hip_buf.h"

static std::string g_error;
void cba::set_error(const std::string& msg) { g_error = msg; }

using cba::DevBuf;
using cba::PinnedBuf;
using cba::span_fits;

static int g_failed = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failed += 1; } \
  } while (0)

// a refusal: CBA_ERR_STATE and the three numbers in the error text
static bool refused(int rc, size_t n, size_t offset, size_t size) {
  const std::string want = std::to_string(n) + " elements at offset " + std::to_string(offset) + " do not fit a buffer of " + std::to_string(size);
  return rc == CBA_ERR_STATE && g_error.find(want) != std::string::npos;
}

static void check_without_device() {
  CHECK(span_fits(8, 8, 0) && !span_fits(8, 9, 0) && span_fits(8, 5, 3) && !span_fits(8, 5, 4));
  CHECK(!span_fits(8, 5, SIZE_MAX - 2) && !span_fits(8, SIZE_MAX, 2) && span_fits(0, 0, 0) && !span_fits(0, 0, 1));
  DevBuf<double> e;
  double h[2] = {1, 2};
  CHECK(e.size() == 0 && (double*)e == nullptr);
  CHECK(refused(e.upload(h, 1), 1, 0, 0) && refused(e.download(h, 2), 2, 0, 0) && refused(e.zero(1), 1, 0, 0));
  CHECK(refused(e.fill_bytes(0xFF, 1, 0), 1, 0, 0) && refused(e.upload_async(h, 1, nullptr), 1, 0, 0) && refused(e.zero(0, 1), 0, 1, 0));
  CHECK(g_error.find("zero") != std::string::npos);                      // the operation is named
  CHECK(e.upload(h, 0) == CBA_OK && e.download(h, 0) == CBA_OK && e.zero() == CBA_OK && e.zero_async(nullptr) == CBA_OK);
  CHECK(e.download_optional(nullptr, 5) == CBA_OK && refused(e.download_optional(h, 1), 1, 0, 0));
  DevBuf<double> other;
  CHECK(refused(e.copy_from_async(other, 1, 0, 0, nullptr), 1, 0, 0) && e.copy_from_async(other, 0, 0, 0, nullptr) == CBA_OK);
  PinnedBuf<double> pin;
  CHECK(refused(e.download_async(pin, 1, nullptr), 1, 0, 0) && e.download_async(pin, 0, nullptr) == CBA_OK);
  CHECK(h[0] == 1 && h[1] == 2);
}

static void check_with_device() {
  DevBuf<double> b;
  CHECK(b.alloc(8) == CBA_OK && b.size() == 8 && (double*)b != nullptr);
  double in[9], out[9];
  for (int i = 0; i < 9; ++i) { in[i] = 1.5 * (i + 1); out[i] = -1; }
  CHECK(b.upload(in, 8) == CBA_OK && b.download(out, 8) == CBA_OK && std::memcmp(in, out, 8 * sizeof(double)) == 0 && out[8] == -1);
  double other[9] = {0};
  CHECK(refused(b.upload(other, 9), 9, 0, 8));
  CHECK(g_error.find("upload") != std::string::npos);
  CHECK(b.download(out, 8) == CBA_OK && std::memcmp(in, out, 8 * sizeof(double)) == 0);      // contents unchanged
  CHECK(b.upload(other, 0, 8) == CBA_OK && b.download(out, 0, 8) == CBA_OK);
  CHECK(refused(b.upload(other, 4, 5), 4, 5, 8) && refused(b.download(out, 4, 5), 4, 5, 8) && refused(b.zero(0, 9), 0, 9, 8));
  CHECK(b.zero(3, 2) == CBA_OK && b.download(out, 8) == CBA_OK);
  for (int i = 0; i < 8; ++i) CHECK(out[i] == ((i >= 2 && i <= 4) ? 0.0 : in[i]));
  CHECK(b.fill_bytes(0xFF, 1, 7) == CBA_OK && b.download(out, 8) == CBA_OK && out[7] != out[7] && out[6] == in[6]);      // all ones: a NaN

  DevBuf<double> z;
  CHECK(z.alloc(0) == CBA_OK && (double*)z != nullptr && z.size() == 0);
  CHECK(z.upload(in, 0) == CBA_OK && refused(z.upload(in, 1), 1, 0, 0));
  CHECK(z.alloc_zero(4) == CBA_OK && z.size() == 4 && z.download(out, 4) == CBA_OK && out[0] == 0 && out[3] == 0);

  DevBuf<int> v;
  const std::vector<int> hv = {3, 1, 4, 1, 5};
  int iv[5] = {0};
  CHECK(v.assign(hv) == CBA_OK && v.size() == 5 && v.download(iv, 5) == CBA_OK && std::memcmp(iv, hv.data(), sizeof(iv)) == 0);
  const int* before = v;
  CHECK(v.reserve(3) == CBA_OK && v.size() == 5 && (const int*)v == before);                  // never shrinks, keeps what fits
  CHECK(v.reserve(5) == CBA_OK && v.size() == 5 && (const int*)v == before);
  CHECK(v.reserve(9) == CBA_OK && v.size() == 9);
  DevBuf<int> r;
  CHECK(r.reserve(0) == CBA_OK && (int*)r != nullptr && r.size() == 0);

  DevBuf<int> moved(std::move(v));
  CHECK(v.size() == 0 && (int*)v == nullptr && moved.size() == 9);
  v = std::move(moved);
  CHECK(moved.size() == 0 && (int*)moved == nullptr && v.size() == 9);
  v.reset();
  CHECK(v.size() == 0 && (int*)v == nullptr);

  PinnedBuf<double> pin;
  CHECK(pin.alloc(8) == CBA_OK && pin.size() == 8);
  CHECK(b.upload(in, 8) == CBA_OK);
  for (int i = 0; i < 8; ++i) pin[i] = -1;
  CHECK(b.download_async(pin, 8, nullptr) == CBA_OK && hipStreamSynchronize(nullptr) == hipSuccess);
  for (int i = 0; i < 8; ++i) CHECK(pin[i] == in[i]);
  CHECK(refused(b.download_async(pin, 8, nullptr, 0, 1), 8, 1, 8));                           // one past the pinned side's length
  CHECK(g_error.find("pinned") != std::string::npos);
  CHECK(refused(b.upload_async(pin, 4, nullptr, 0, 5), 4, 5, 8) && refused(b.upload_async(pin, 4, nullptr, 5, 0), 4, 5, 8));
  pin[1] = 42;
  CHECK(b.upload_async(pin, 1, nullptr, 3, 1) == CBA_OK && b.download_sync(out, 8, nullptr) == CBA_OK && out[3] == 42 && out[2] == in[2]);

  DevBuf<double> src;
  CHECK(src.assign(in, 4) == CBA_OK);
  CHECK(refused(b.copy_from_async(src, 5, 0, 0, nullptr), 5, 0, 4));                          // the source does not fit
  CHECK(refused(b.copy_from_async(src, 4, 5, 0, nullptr), 4, 5, 8));                          // the destination does not fit
  CHECK(b.zero() == CBA_OK && b.copy_from_async(src, 2, 6, 1, nullptr) == CBA_OK && b.download_sync(out, 8, nullptr) == CBA_OK);
  CHECK(out[5] == 0 && out[6] == in[1] && out[7] == in[2]);
}

int main(int argc, char** argv) {
  const bool no_device = argc > 1 && std::strcmp(argv[1], "--no-device") == 0;
  check_without_device();
  if (!no_device) check_with_device();
  std::printf("hip_buf_check%s: %s\n", no_device ? " --no-device" : "", g_failed ? "FAILED" : "ok");
  return g_failed ? 1 : 0;
}
