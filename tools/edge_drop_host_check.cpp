// Stand-alone host check of mgcn_edge_drop_records_host (csrc/dropout.hip) and mgcn_edge_drop_table_host (csrc/csr_build.cpp) for a host
// sanitizer run (include/mgcn_hip.h (19)): a small mirrored graph with self edges, duplicate triples, an isolated node and hubs of
// several chunks is laid out by mgcn_csr_build_host into exactly-sized heap blocks; the twin then rewrites the records for a grid of
// thresholds with and without forced edges, and every kept slot's norm is compared, bit for bit, with the norm the feeder folds when
// it is run on the kept edge list alone. No GPU call is made.
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//     tools/edge_drop_host_check.cpp kgc-gcn_amd/csrc/dropout.hip kgc-gcn_amd/csrc/csr_build.cpp -o edge_drop_host_check
//   ./edge_drop_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/mgcn_hip.h"

namespace {

struct Layout {
  std::vector<int32_t> rowptr, hubinfo, chunks, slot_dst, mirror, typeptr, typeslots;
  std::vector<mgcn_edge_rec> rec;
  std::vector<int64_t> perm;
  int64_t num_chunks = 0;
};

bool build(int64_t N, int64_t R, const std::vector<int64_t> &s, const std::vector<int64_t> &o, const std::vector<int64_t> &r, int64_t thr,
           int64_t chunk, Layout &L) {
  const int64_t E = int64_t(s.size()), E2 = 2 * E;
  std::vector<int64_t> ei(size_t(2 * E2)), et(static_cast<size_t>(E2));      // (size 0 stays a valid pointer-free vector: E > 0 here)
  for (int64_t e = 0; e < E; ++e) {
    ei[e] = s[e], ei[E + e] = o[e], ei[E2 + e] = o[e], ei[E2 + E + e] = s[e];
    et[e] = r[e], et[E + e] = r[e] + R;
  }
  const int64_t max_chunks = thr > 0 ? E2 / chunk + E2 / thr + 2 : 0;
  L.rowptr.assign(size_t(2 * (N + 1)), 0), L.hubinfo.assign(size_t(4 * N), 0), L.chunks.assign(size_t(4 * (max_chunks > 0 ? max_chunks : 1)), 0);
  L.rec.resize(size_t(E2)), L.perm.resize(size_t(E2)), L.slot_dst.resize(size_t(E2)), L.mirror.resize(size_t(E2));
  L.typeptr.resize(size_t(2 * R + 2)), L.typeslots.resize(size_t(E2));
  return mgcn_csr_build_host(N, E, 2 * R + 1, ei.data(), et.data(), thr, chunk, L.rowptr.data(), L.rec.data(), L.perm.data(), L.hubinfo.data(),
                             L.chunks.data(), max_chunks, &L.num_chunks, L.slot_dst.data(), L.mirror.data(), L.typeptr.data(),
                             L.typeslots.data()) == MGCN_OK;
}

int fail(const char *what) {
  std::fprintf(stderr, "edge drop host check: %s (%s)\n", what, mgcn_last_error());
  return 1;
}

}  // namespace

int main() {
  const int64_t N = 23, R = 2;
  std::vector<int64_t> s, o, r;
  for (int k = 0; k < 37; ++k) s.push_back(3 + (5 * k) % 17), o.push_back(0), r.push_back(k % R);      // node 0: a hub of many chunks
  for (int k = 0; k < 9; ++k) s.push_back(1), o.push_back(3 + k), r.push_back(1);                      // node 1 leaves nine edges
  for (int k = 0; k < 20; ++k) s.push_back((7 * k + 2) % 21), o.push_back((11 * k + 5) % 21), r.push_back(k % R);
  s.push_back(4), o.push_back(4), r.push_back(0);                                                      // a self edge, twice
  s.push_back(4), o.push_back(4), r.push_back(0);
  s.push_back(0), o.push_back(2), r.push_back(1);                                                      // (node 22 stays isolated)
  const int64_t E = int64_t(s.size()), E2 = 2 * E;
  long checked = 0;
  for (int64_t thr : {int64_t(0), int64_t(1), int64_t(4)}) {
    Layout L;
    if (!build(N, R, s, o, r, thr, 2, L)) return fail("csr_build refused the graph");
    int64_t max_run = 0;
    for (int h = 0; h < 2; ++h)
      for (int64_t n = 0; n < N; ++n) {
        int64_t len = L.rowptr[size_t(h * (N + 1) + n + 1)] - L.rowptr[size_t(h * (N + 1) + n)];
        const int64_t first = L.hubinfo[size_t((h * N + n) * 2)], cnt = L.hubinfo[size_t((h * N + n) * 2 + 1)];
        if (cnt > 0) len = L.chunks[size_t((first + cnt - 1) * 4 + 1)] - L.chunks[size_t(first * 4)];
        if (len > max_run) max_run = len;
      }
    std::vector<float> table(size_t(max_run + 1));
    if (mgcn_edge_drop_table_host(max_run + 1, table.data()) != MGCN_OK) return fail("table refused");
    if (table[0] != 0.0f || table[1] != 1.0f) return fail("table[0], table[1]");
    const int32_t *hubinfo = L.num_chunks ? L.hubinfo.data() : nullptr, *chunks = L.num_chunks ? L.chunks.data() : nullptr;
    // a table one entry short is refused and nothing is written
    {
      std::vector<float> shorter(table.begin(), table.end() - 1), cinv(size_t(2 * N), -1.f);
      std::vector<mgcn_edge_rec> out(static_cast<size_t>(E2));
      std::memset(out.data(), 0x5A, sizeof(mgcn_edge_rec) * out.size());
      if (max_run > 0 && mgcn_edge_drop_records_host(N, E, L.rowptr.data(), L.rec.data(), L.slot_dst.data(), hubinfo, chunks, L.num_chunks, shorter.data(),
                                                     max_run, nullptr, 1, 1u << 31, cinv.data(), out.data()) != MGCN_EINVAL)
        return fail("a short table was accepted");
      if (cinv[0] != -1.f || out[0].src != 0x5A5A5A5A) return fail("a refused call wrote");
    }
    for (uint32_t threshold : {0u, 1u << 30, 1u << 31, 3435973836u, 0xffffffffu})
      for (int with_forced = 0; with_forced < 3; ++with_forced) {
        std::vector<uint8_t> forced(size_t(E), 0);
        if (with_forced == 1)
          for (int64_t u = 0; u < E; u += 3) forced[size_t(u)] = 1;
        if (with_forced == 2)                                                   // node 0 loses every edge
          for (int64_t u = 0; u < E; ++u) forced[size_t(u)] = s[size_t(u)] == 0 || o[size_t(u)] == 0;
        std::vector<float> cinv(size_t(2 * N));
        std::vector<mgcn_edge_rec> out(static_cast<size_t>(E2));
        const uint64_t key = 0x9e3779b97f4a7c15ull * (threshold | 1u);
        if (mgcn_edge_drop_records_host(N, E, L.rowptr.data(), L.rec.data(), L.slot_dst.data(), hubinfo, chunks, L.num_chunks, table.data(),
                                        max_run + 1, with_forced ? forced.data() : nullptr, key, threshold, cinv.data(), out.data()) != MGCN_OK)
          return fail("the twin refused");
        // the kept list, from the mask of (12) and the forced bytes (a kept edge may still carry norm 0: a leaf destination)
        std::vector<uint8_t> kept(static_cast<size_t>(E));
        if (mgcn_dropout_mask_host(E, 1, kept.data(), 1, key, 0, threshold) != MGCN_OK) return fail("mask refused");
        if (with_forced)
          for (int64_t u = 0; u < E; ++u) kept[size_t(u)] = kept[size_t(u)] && !forced[size_t(u)];
        std::vector<int64_t> ks, ko, kr, kid;
        std::vector<float> norm_of(size_t(E2), 0.f);
        for (int64_t p = 0; p < E2; ++p) {
          const mgcn_edge_rec &a = L.rec[size_t(p)], &b = out[size_t(p)];
          if (a.src != b.src || a.type != b.type || a.eid != b.eid) return fail("src / type / eid changed");
          if (!(b.norm >= 0.f) || b.norm > 1.f || (b.norm == 0.f && std::signbit(b.norm))) return fail("a norm outside [+0, 1]");
          norm_of[size_t(b.eid)] = b.norm;
        }
        for (int64_t u = 0; u < E; ++u) {
          if (!kept[size_t(u)] && (norm_of[size_t(u)] != 0.f || norm_of[size_t(u + E)] != 0.f)) return fail("a dropped edge carries a norm");
          if (threshold == 0 && kept[size_t(u)]) return fail("threshold 0 kept an edge");
          if (kept[size_t(u)]) ks.push_back(s[size_t(u)]), ko.push_back(o[size_t(u)]), kr.push_back(r[size_t(u)]), kid.push_back(u);
        }
        if (with_forced == 2 && (cinv[0] != 0.f || cinv[size_t(N)] != 0.f)) return fail("a node without edges kept a degree");
        if (!ks.empty()) {
          Layout K;
          if (!build(N, R, ks, ko, kr, 0, 2, K)) return fail("csr_build refused the kept list");
          const int64_t Ek = int64_t(ks.size());
          for (int64_t p = 0; p < 2 * Ek; ++p) {
            const mgcn_edge_rec &k = K.rec[size_t(p)];
            const int64_t orig = k.eid < Ek ? kid[size_t(k.eid)] : kid[size_t(k.eid - Ek)] + E;
            if (std::memcmp(&k.norm, &norm_of[size_t(orig)], sizeof(float)) != 0) return fail("a kept norm is not the feeder's on the kept list");
          }
        }
        ++checked;
      }
  }
  // refusals
  float one = 0.f;
  if (mgcn_edge_drop_table_host(0, &one) != MGCN_EINVAL || mgcn_edge_drop_table_host(2, nullptr) != MGCN_EINVAL) return fail("table refusals");
  std::printf("edge drop host check ok: %ld grid points, E = %lld\n", checked, (long long)E);
  return 0;
}
