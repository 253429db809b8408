// Error paths of csrc/device_call.h, which no GPU test can reach: the real header over the stand-in runtime of
// hip/hip_runtime.h (next to this file), with a failure injected at every runtime call in turn.  Built with
// -fsanitize=address,undefined by tests/test_device_call_cpu.py; exits 0 when every check holds.
#include <cstdio>
#include <vector>

#include "device_call.h"

using namespace lc;

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);             \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

constexpr size_t kCount = 5;

// an entry point in small: one input, a mandatory and an optional output; the "kernel" runs on the host
static int small_call(lc_ctx *ctx, const float *in, float *twice, float *plus_one, float *kernel_ms) {
  LC_ENTER(ctx);
  DeviceCall call(ctx);
  const float *d_in = nullptr;
  float *d_twice = nullptr, *d_plus = nullptr;
  LC_HIP(ctx, call.upload(in, kCount, &d_in));
  LC_HIP(ctx, call.result(twice, kCount, &d_twice));
  LC_HIP(ctx, call.result(plus_one, kCount, &d_plus));
  LC_HIP(ctx, call.start());
  for (size_t i = 0; i < kCount; ++i) {
    d_twice[i] = 2.f * d_in[i];
    if (d_plus) d_plus[i] = d_in[i] + 1.f;
  }
  LC_HIP(ctx, call.stop());
  LC_HIP(ctx, call.finish(kernel_ms));
  return LC_OK;
}

static void test_call() {
  lc_ctx ctx;
  const float in[kCount] = {1.f, 2.f, 3.f, 4.f, 5.f};
  float twice[kCount] = {}, plus[kCount] = {}, ms = 0.f;
  fake_hip::reset(0);
  CHECK(small_call(&ctx, in, twice, plus, &ms) == LC_OK);
  const int n_calls = fake_hip::calls, n_mallocs = fake_hip::mallocs;
  CHECK(n_calls == 11 && n_mallocs == 3);  // set device, 3 allocations, 1 + 2 copies, 2 events, synchronise, elapsed
  CHECK(fake_hip::live == 0 && ms == 0.25f);
  for (size_t i = 0; i < kCount; ++i) CHECK(twice[i] == 2.f * in[i] && plus[i] == in[i] + 1.f);
  for (int k = 1; k <= n_calls; ++k) {
    ctx.err.clear();
    fake_hip::reset(k);
    CHECK(small_call(&ctx, in, twice, plus, &ms) == LC_ERR_DEVICE);
    CHECK(fake_hip::calls == k);  // nothing is enqueued after the failure
    CHECK(!ctx.err.empty() && fake_hip::live == 0);
  }
  // without the optional output and the time: one buffer, one copy and the elapsed-time call fewer
  float twice2[kCount] = {};
  fake_hip::reset(0);
  CHECK(small_call(&ctx, in, twice2, nullptr, nullptr) == LC_OK);
  CHECK(fake_hip::mallocs == n_mallocs - 1 && fake_hip::calls == n_calls - 3 && fake_hip::live == 0);
  for (size_t i = 0; i < kCount; ++i) CHECK(twice2[i] == twice[i]);
  // a null input gives a null device pointer and allocates nothing
  {
    DeviceCall call(&ctx);
    const float *d = in;
    fake_hip::reset(0);
    CHECK(call.upload((const float *)nullptr, kCount, &d) == hipSuccess && d == nullptr && fake_hip::calls == 0);
  }
}

static int grow(lc_ctx *ctx, float **hist, int *stride, int rows, int needed) {
  LC_HIP(ctx, grow_history(hist, stride, rows, needed, ctx->stream));
  return LC_OK;
}

// rows x stride values, hist[r][c] = 100 r + c + 1, grown first from nothing and then from what is there
static void test_grow(int rows) {
  lc_ctx ctx;
  float *hist = nullptr;
  int stride = 0;
  const int needed[2] = {10, 100}, expect[2] = {64, 192}, clean_calls[2] = {2, 4};
  for (int step = 0; step < 2; ++step) {
    float *const old = hist;
    const int old_stride = stride, live = fake_hip::live;
    for (int k = 1; k <= clean_calls[step]; ++k) {
      ctx.err.clear();
      fake_hip::reset(k);
      CHECK(grow(&ctx, &hist, &stride, rows, needed[step]) == LC_ERR_DEVICE && !ctx.err.empty());
      CHECK(hist == old && stride == old_stride && fake_hip::live == live);
      for (int r = 0; r < rows && old; ++r)
        for (int c = 0; c < old_stride; ++c) CHECK(old[(size_t)r * old_stride + c] == (float)(100 * r + c + 1));
    }
    std::vector<float> before(old, old + (size_t)rows * old_stride);
    fake_hip::reset(0);
    CHECK(grow(&ctx, &hist, &stride, rows, needed[step]) == LC_OK);
    CHECK(fake_hip::calls == clean_calls[step] && stride == expect[step] && fake_hip::live == 1);
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < stride; ++c)
        CHECK(hist[(size_t)r * stride + c] == (c < old_stride ? before[(size_t)r * old_stride + c] : 0.f));
    fake_hip::reset(0);
    CHECK(grow(&ctx, &hist, &stride, rows, stride) == LC_OK && fake_hip::calls == 0);  // large enough: nothing to do
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < stride; ++c) hist[(size_t)r * stride + c] = (float)(100 * r + c + 1);
  }
  (void)hipFree(hist);
  CHECK(fake_hip::live == 0);
}

static void test_pool() {
  float *a = nullptr;
  double *b = nullptr;
  {
    DevPool pool;
    fake_hip::reset(0);
    CHECK(pool.alloc(3, &a) == hipSuccess && pool.alloc_zeroed(4, &b, nullptr) == hipSuccess && fake_hip::live == 2);
    for (int i = 0; i < 4; ++i) CHECK(b[i] == 0.0);
    fake_hip::reset(2);  // the allocation succeeds, the fill fails: the pool still owns the buffer
    CHECK(pool.alloc_zeroed(4, &b, nullptr) == hipErrorUnknown && fake_hip::live == 3);
    fake_hip::reset(1);
    CHECK(pool.alloc(3, &a) == hipErrorOutOfMemory && fake_hip::live == 3);
  }
  CHECK(fake_hip::live == 0);
}

int main() {
  test_call();
  test_grow(3);
  test_grow(1);
  test_pool();
  if (failures) return 1;
  std::printf("device_call: all checks passed\n");
  return 0;
}
