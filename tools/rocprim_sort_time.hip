// rocprim_sort_time.hip — the yardstick of the ray order's radix sort (rt_order.hip):
// rocprim::radix_sort_pairs of (uint32 key, uint32 index) over key bits [0, 32) on a key set written
// by tools/order_time.py --keys-dir.  Built in a measuring session only, where rocPRIM's headers
// exist; never linked into the library.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/rocprim_sort_time.hip -o rocprim_sort_time
//   rocprim_sort_time keys_1048576.bin [reps]
// Prints one JSON line: the median, minimum and maximum of `reps` timed sorts after two warm-up
// sorts, HIP events on the null stream, the temporary storage allocated once before.
#include <hip/hip_runtime.h>

#include <cstring>  // (rocPRIM's texture iterator calls memset)

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                          \
  do {                                                                    \
    hipError_t e_ = (x);                                                  \
    if (e_ != hipSuccess) {                                               \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));        \
      return 1;                                                           \
    }                                                                     \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const int reps = argc > 2 ? std::atoi(argv[2]) : 7;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::fseek(f, 0, SEEK_END);
  const size_t n = (size_t)std::ftell(f) / sizeof(uint32_t);
  std::fseek(f, 0, SEEK_SET);
  std::vector<uint32_t> keys(n), vals(n);
  if (std::fread(keys.data(), sizeof(uint32_t), n, f) != n) return 2;
  std::fclose(f);
  for (size_t i = 0; i < n; ++i) vals[i] = (uint32_t)i;
  uint32_t *d_k, *d_v, *d_ko, *d_vo;
  CHECK(hipMalloc(&d_k, n * 4));
  CHECK(hipMalloc(&d_v, n * 4));
  CHECK(hipMalloc(&d_ko, n * 4));
  CHECK(hipMalloc(&d_vo, n * 4));
  CHECK(hipMemcpy(d_k, keys.data(), n * 4, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_v, vals.data(), n * 4, hipMemcpyHostToDevice));
  size_t tmp_bytes = 0;
  CHECK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, d_k, d_ko, d_v, d_vo, n, 0, 32));
  void* tmp = nullptr;
  CHECK(hipMalloc(&tmp, tmp_bytes ? tmp_bytes : 16));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  std::vector<float> ms;
  for (int r = 0; r < reps + 2; ++r) {
    CHECK(hipEventRecord(e0, nullptr));
    CHECK(rocprim::radix_sort_pairs(tmp, tmp_bytes, d_k, d_ko, d_v, d_vo, n, 0, 32));
    CHECK(hipEventRecord(e1, nullptr));
    CHECK(hipEventSynchronize(e1));
    float t = 0;
    CHECK(hipEventElapsedTime(&t, e0, e1));
    if (r >= 2) ms.push_back(t);
  }
  // the result is the stable order
  CHECK(hipMemcpy(vals.data(), d_vo, n * 4, hipMemcpyDeviceToHost));
  bool ok = true;
  for (size_t i = 1; i < n && ok; ++i)
    ok = keys[vals[i - 1]] < keys[vals[i]] || (keys[vals[i - 1]] == keys[vals[i]] && vals[i - 1] < vals[i]);
  std::sort(ms.begin(), ms.end());
  std::printf("{\"kind\": \"rocprim_sort\", \"pairs\": %zu, \"ms\": %.4f, \"min\": %.4f, \"max\": %.4f, \"stable_order\": %s}\n", n,
              ms[ms.size() / 2], ms.front(), ms.back(), ok ? "true" : "false");
  return ok ? 0 : 1;
}
