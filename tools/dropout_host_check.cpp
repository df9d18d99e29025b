// Stand-alone host check of mgcn_dropout_mask_host (csrc/dropout.hip) for a host sanitizer run: walks the tests' grid of rows, columns,
// leading dimensions, first rows and thresholds into exactly-sized heap blocks, checks that padding bytes stay untouched, that a row
// slice equals the whole block's rows, and the definition's pinned bits (include/mgcn_hip.h (12)). No GPU call is made.
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//     tools/dropout_host_check.cpp kgc-gcn_amd/csrc/dropout.hip kgc-gcn_amd/csrc/csr_build.cpp -o dropout_host_check
//   ./dropout_host_check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/mgcn_hip.h"

int main() {
  const int64_t rows_grid[] = {1, 63, 64, 65, 257};
  const int32_t cols_grid[] = {1, 3, 4, 5, 100, 200, 201};
  const uint64_t row0_grid[] = {0, 7, (uint64_t(1) << 32) - 3, (uint64_t(1) << 40) + 1};
  const uint32_t thr_grid[] = {3865470566u, 3006477107u, 2147483648u, 0u, 0xffffffffu};
  const uint64_t key = 0x2bbde2bebe8ae998ull;   // key(1234, 5, 0x1001)
  long checked = 0;
  for (int64_t rows : rows_grid)
    for (int32_t cols : cols_grid)
      for (int64_t pad : {0, 1, 4})
        for (uint64_t row0 : row0_grid)
          for (uint32_t thr : thr_grid) {
            const int64_t ld = cols + pad;
            std::vector<uint8_t> whole(size_t(rows * ld), 0xAA);
            if (mgcn_dropout_mask_host(rows, cols, whole.data(), ld, key, row0, thr) != MGCN_OK) {
              std::fprintf(stderr, "refused: %s\n", mgcn_last_error());
              return 1;
            }
            for (int64_t r = 0; r < rows; ++r)
              for (int64_t c = 0; c < ld; ++c) {
                const uint8_t v = whole[size_t(r * ld + c)];
                if (c < cols ? v > 1 : v != 0xAA) {
                  std::fprintf(stderr, "bad byte %u at (%lld, %lld)\n", v, (long long)r, (long long)c);
                  return 1;
                }
              }
            // rows [a, rows) launched with row0 + a equal that slice
            const int64_t a = rows / 2;
            std::vector<uint8_t> part(size_t((rows - a) * cols));
            if (rows - a > 0) {
              if (mgcn_dropout_mask_host(rows - a, cols, part.data(), cols, key, row0 + uint64_t(a), thr) != MGCN_OK) return 1;
              for (int64_t r = a; r < rows; ++r)
                if (std::memcmp(&part[size_t((r - a) * cols)], &whole[size_t(r * ld)], size_t(cols)) != 0) {
                  std::fprintf(stderr, "slice differs at row %lld\n", (long long)r);
                  return 1;
                }
            }
            ++checked;
          }
  // pinned bits: key(1234, 5, 0x1001), p = 0.3
  uint8_t bits[12];
  const char *want[2] = {"011111011010", "111010111101"};
  const uint64_t pin_row0[2] = {0, (uint64_t(1) << 32) + 7};
  for (int i = 0; i < 2; ++i) {
    if (mgcn_dropout_mask_host(1, 12, bits, 12, key, pin_row0[i], 3006477107u) != MGCN_OK) return 1;
    for (int c = 0; c < 12; ++c)
      if (bits[c] != uint8_t(want[i][c] - '0')) {
        std::fprintf(stderr, "pinned bits differ (row0 %d, column %d)\n", i, c);
        return 1;
      }
  }
  // refusals write nothing and set the message
  if (mgcn_dropout_mask_host(2, 4, nullptr, 4, key, 0, 1) != MGCN_EINVAL || mgcn_dropout_mask_host(2, 4, bits, 3, key, 0, 1) != MGCN_EINVAL ||
      mgcn_dropout_mask_host(-1, 4, bits, 4, key, 0, 1) != MGCN_EINVAL || mgcn_dropout_mask_host(2, 0, bits, 4, key, 0, 1) != MGCN_EINVAL)
    return 1;
  std::printf("dropout host check ok: %ld grid points\n", checked);
  return 0;
}
