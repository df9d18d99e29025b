// Stand-alone host check of mgcn_alias_build_host (csrc/csr_build.cpp) and mgcn_cand_draw_alias_host (csrc/dropout.hip) for a host
// sanitizer run: builds tables of the tests' weight shapes into exactly-sized heap blocks, checks every alias and the sum of the
// counts (include/mgcn_hip.h (17)), draws lists through them into padded blocks whose padding must stay untouched, draws through a
// corrupt table (every written id is -1 or inside the table), and checks that the equal-weights table gives mgcn_cand_draw_host's
// block. No GPU call is made.
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//     tools/alias_host_check.cpp kgc-gcn_amd/csrc/dropout.hip kgc-gcn_amd/csrc/csr_build.cpp -o alias_host_check
//   ./alias_host_check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/mgcn_hip.h"

static int fail(const char *what) {
  std::fprintf(stderr, "alias host check: %s (%s)\n", what, mgcn_last_error());
  return 1;
}

int main() {
  const uint64_t key = 0x3240e6b5af382cbdull;      // key(1234, 5, 0x2000)
  const std::vector<int64_t> keys = {10, 20, 30, 40}, ptr = {0, 1, 4, 4, 9}, qk = {20, 10, 40, 5, 30, 25, 99};
  const std::vector<int32_t> tails = {5, 0, 3, 6, 1, 2, 4, 5, 6};
  long tables = 0, blocks = 0;
  for (int64_t N : {int64_t(1), int64_t(2), int64_t(5), int64_t(8), int64_t(4097)})
    for (int shape = 0; shape < 4; ++shape) {
      std::vector<int64_t> w(static_cast<size_t>(N));
      for (int64_t n = 0; n < N; ++n)
        w[size_t(n)] = shape == 0 ? 7 : shape == 1 ? n + 1 : shape == 2 ? (n == N / 2 ? 4 : 0) : (n % 3 ? int64_t(1048576.0 / double(n + 1)) + 1 : 0);
      if (shape == 3 && N == 1) w[0] = (int64_t(1) << 32) - 1;
      std::vector<int64_t> table(static_cast<size_t>(N), -77);
      if (mgcn_alias_build_host(N, w.data(), table.data()) != MGCN_OK) return fail("build refused");
      std::vector<uint64_t> cnt(static_cast<size_t>(N), 0);      // (N <= 4097 here: N 2^32 fits 64 bits)
      for (int64_t n = 0; n < N; ++n) {
        const uint64_t t = uint64_t(table[size_t(n)]), alias = t >> 32, thr = t & 0xffffffffull;
        if (alias >= uint64_t(N)) return fail("alias outside the table");
        if (shape == 0 && t != (uint64_t(n) << 32 | 0xffffffffull)) return fail("equal weights: not the identity table");
        cnt[size_t(n)] += thr;                                   // thr to the slot itself, 2^32 - thr to its alias
        cnt[size_t(alias)] += (uint64_t(1) << 32) - thr;
      }
      uint64_t sum = 0;
      for (int64_t n = 0; n < N; ++n) {
        if (w[size_t(n)] == 0 && cnt[size_t(n)] != 0) return fail("an entity of weight zero has a count");
        sum += cnt[size_t(n)];
      }
      if (sum != uint64_t(N) << 32) return fail("the counts do not sum to N 2^32");
      ++tables;
      for (int64_t B : {int64_t(1), int64_t(7)})
        for (int64_t K : {int64_t(1), int64_t(2), int64_t(3), int64_t(65)})
          for (int64_t pad : {int64_t(0), int64_t(3)})
            for (int labels = 0; labels < 2; ++labels) {
              const int64_t ld = K + pad;
              std::vector<int64_t> cand(size_t(B * ld), -77), uni(size_t(B * ld), -77);
              std::vector<uint8_t> label(size_t(B * ld), 0xAA);
              if (mgcn_cand_draw_alias_host(B, K, N, qk.data(), 4, keys.data(), ptr.data(), tails.data(), 9, table.data(), key,
                                            (uint64_t(1) << 32) + 5, cand.data(), ld, labels ? label.data() : nullptr, labels ? ld : 0) != MGCN_OK)
                return fail("draw refused");
              for (int64_t b = 0; b < B; ++b)
                for (int64_t j = 0; j < ld; ++j) {
                  const int64_t v = cand[size_t(b * ld + j)];
                  if (j >= K ? v != -77 : (j >= 1 && (v < 0 || v >= N))) return fail("bad id or touched padding");
                  if (j >= 1 && j < K && w[size_t(v)] == 0) return fail("an entity of weight zero was drawn");
                  const uint8_t l = label[size_t(b * ld + j)];
                  if (labels && j < K ? l > 1 : l != 0xAA) return fail("bad label or touched padding");
                }
              if (shape == 0) {
                if (mgcn_cand_draw_host(B, K, N, qk.data(), 4, keys.data(), ptr.data(), tails.data(), 9, key, (uint64_t(1) << 32) + 5,
                                        uni.data(), ld, nullptr, 0) != MGCN_OK)
                  return fail("uniform draw refused");
                if (std::memcmp(uni.data(), cand.data(), uni.size() * sizeof(int64_t)) != 0) return fail("equal weights: not the uniform block");
              }
              ++blocks;
            }
    }
  // a corrupt table: aliases of N, -1 and 2^31 with threshold 0: -1 is written, nothing outside the table is followed
  {
    const int64_t N = 4;
    const std::vector<int64_t> bad = {int64_t(N) << 32, int64_t(uint64_t(0xffffffffull) << 32), int64_t(uint64_t(1) << 63), int64_t(2) << 32};
    std::vector<int64_t> cand(7 * 65, -77);
    if (mgcn_cand_draw_alias_host(7, 65, N, qk.data(), 4, keys.data(), ptr.data(), tails.data(), 9, bad.data(), key, 0, cand.data(), 65,
                                  nullptr, 0) != MGCN_OK)
      return fail("corrupt table refused");
    long dead = 0;
    for (int64_t b = 0; b < 7; ++b)
      for (int64_t j = 1; j < 65; ++j) {
        const int64_t v = cand[size_t(b * 65 + j)];
        if (v != -1 && v != 2) return fail("corrupt table: an id that is neither -1 nor the one good alias");
        dead += v == -1;
      }
    if (!dead) return fail("corrupt table: no dead position");
  }
  // refusals write nothing and set the message
  {
    std::vector<int64_t> w = {1, 2, 3}, table(3, -77), cand(8, -77);
    int64_t neg[3] = {1, -1, 3}, big[3] = {1, int64_t(1) << 32, 3}, zero[3] = {0, 0, 0};
    if (mgcn_alias_build_host(3, nullptr, table.data()) != MGCN_EINVAL || mgcn_alias_build_host(3, w.data(), nullptr) != MGCN_EINVAL ||
        mgcn_alias_build_host(0, w.data(), table.data()) != MGCN_EINVAL || mgcn_alias_build_host(int64_t(1) << 31, w.data(), table.data()) != MGCN_EINVAL ||
        mgcn_alias_build_host(3, neg, table.data()) != MGCN_EINVAL || mgcn_alias_build_host(3, big, table.data()) != MGCN_EINVAL ||
        mgcn_alias_build_host(3, zero, table.data()) != MGCN_EINVAL)
      return fail("a bad build was not refused");
    if (mgcn_cand_draw_alias_host(1, 8, 3, qk.data(), 4, keys.data(), ptr.data(), tails.data(), 9, nullptr, key, 0, cand.data(), 8, nullptr, 0) != MGCN_EINVAL ||
        mgcn_cand_draw_alias_host(1, 8, 3, qk.data(), 4, keys.data(), ptr.data(), tails.data(), 9,
                                  reinterpret_cast<const int64_t *>(reinterpret_cast<const char *>(w.data()) + 4), key, 0, cand.data(), 8, nullptr, 0) != MGCN_EINVAL ||
        mgcn_cand_draw_alias_host(1, 8, int64_t(1) << 31, qk.data(), 4, keys.data(), ptr.data(), tails.data(), 9, w.data(), key, 0, cand.data(), 8, nullptr, 0) != MGCN_EINVAL)
      return fail("a bad draw was not refused");
    for (int64_t v : table)
      if (v != -77) return fail("a refusal wrote the table");
    for (int64_t v : cand)
      if (v != -77) return fail("a refusal wrote the list");
  }
  std::printf("alias host check ok: %ld tables, %ld blocks\n", tables, blocks);
  return 0;
}
