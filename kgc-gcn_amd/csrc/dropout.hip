// Counter-based dropout (include/mgcn_hip.h (12)): the keep bit of element (row, col) of a site is a pure function of
// (key, global row, col) -- Philox4x32-10 keyed by a SplitMix64 mix of (seed, step, site) that the host computes -- so a mask does
// not depend on the launch geometry, on the rank count or on which rank owns the row, and the backward recomputes it instead of
// loading a saved one. Streaming kernels: one Philox call serves four columns, one lane moves one 16-byte group when base pointers
// and leading dimensions allow it and takes the element-wise path otherwise (same bits). No atomics, no LDS, no inline assembly;
// all index arithmetic is 64-bit.
// The same Philox function also draws the candidate lists of sampled-negative training (include/mgcn_hip.h (15)):
// mgcn_cand_draw, its device-key form and its host twin, at the end of the anonymous namespace, and their weighted forms
// (include/mgcn_hip.h (17)), which read one alias-table word per negative.
// And its keep bits decide which edges a training step's graph keeps (include/mgcn_hip.h (19)): mgcn_edge_drop_records,
// its device-key form and host twin rewrite the slot records' norms for the kept edge list, mgcn_edge_flags_from_queries marks the
// edges that answer the batch's own queries; after the draw kernels in the anonymous namespace.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "mgcn_common.h"

namespace {

constexpr int TPB = 256;            // four waves
constexpr int64_t MAX_BLOCKS = 2048;   // 256 CUs x 8 workgroups; the rest is strided over
constexpr int64_t MAX_ROWS = int64_t(1) << 40;

// The four 32-bit words of column block `cb` (columns 4 cb .. 4 cb + 3) of global row `row` under `key`: Philox4x32-10 with the
// Random123 constants, key words (key & 0xffffffff, key >> 32), counter (row_lo, row_hi, cb, 0). Element (row, col) uses word col & 3.
// The ONE definition: the kernels and mgcn_dropout_mask_host both call it.
__host__ __device__ inline void dropout_words(uint64_t key, uint64_t row, uint32_t cb, uint32_t w[4]) {
  uint32_t k0 = uint32_t(key), k1 = uint32_t(key >> 32);
  uint32_t c0 = uint32_t(row), c1 = uint32_t(row >> 32), c2 = cb, c3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint64_t p0 = uint64_t(0xD2511F53u) * c0, p1 = uint64_t(0xCD9E8D57u) * c2;
    const uint32_t n0 = uint32_t(p1 >> 32) ^ c1 ^ k0, n2 = uint32_t(p0 >> 32) ^ c3 ^ k1;
    c1 = uint32_t(p1);
    c3 = uint32_t(p0);
    c0 = n0;
    c2 = n2;
  }
  w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// One SplitMix64 step (include/mgcn_hip.h (12)), the ONE definition in C++: key(seed, step, site) = sm(sm(sm(seed) ^ step) ^ site).
// The by-value entry points receive the finished key; the _dev ones receive the site id and a pointer to the step word
// sm(sm(seed) ^ step), and every lane forms the last step itself (site_key below), so a captured launch follows the word in memory.
__host__ __device__ inline uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  uint64_t z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the key of a site: `k` itself (KD false: it is the key), or sm(*step_key ^ k) (KD true: k is the site id)
template <bool KD>
__host__ __device__ inline uint64_t site_key(uint64_t k, const uint64_t *step_key) {
  return KD ? splitmix64(*step_key ^ k) : k;
}

// kept: one f32 multiply; dropped: +0.0f whatever x holds (inf and NaN included)
__device__ inline float dropped(float x, bool keep, float inv_keep) { return keep ? x * inv_keep : 0.f; }

// work unit u -> (row, column block); the 32-bit division where u allows it
__device__ inline void unit_of(int64_t u, int32_t ncb, int64_t &r, int32_t &cb) {
  if (u <= int64_t(0xffffffffu)) {
    const uint32_t q = uint32_t(u) / uint32_t(ncb);
    r = q;
    cb = int32_t(uint32_t(u) - q * uint32_t(ncb));
  } else {
    r = u / ncb;
    cb = int32_t(u - r * ncb);
  }
}

struct Site {
  const float *x;
  int64_t ldx;
  float *out;
  int64_t ldo;
  uint64_t key;      // the site's key, or its site id in the _dev entry points
};

// NS sites (1: apply, 2: the layer's in / out pair) over the same [rows, cols] block; VEC: every base pointer is 16-byte aligned and
// every leading dimension a multiple of four floats, so a whole column block is one 16-byte access. A lane reads its elements of
// every site before it writes any, and no lane touches another's elements: an output may be its own input, and the two inputs of a
// pair may be one tensor.
template <int NS, bool VEC, bool KD>
__global__ __launch_bounds__(TPB) void apply_kernel(int64_t rows, int32_t cols, int32_t ncb, Site s0, Site s1, uint64_t row0,
                                                    uint32_t threshold, float inv_keep, const uint64_t *__restrict__ step_key) {
  const int64_t units = rows * ncb, stride = int64_t(gridDim.x) * TPB;
  const uint64_t keys[2] = {site_key<KD>(s0.key, step_key), site_key<KD>(s1.key, step_key)};
  for (int64_t u = int64_t(blockIdx.x) * TPB + threadIdx.x; u < units; u += stride) {
    int64_t r;
    int32_t cb;
    unit_of(u, ncb, r, cb);
    const int32_t c = cb * 4, n = cols - c < 4 ? cols - c : 4;
    const Site site[2] = {s0, s1};
    float v[NS][4];
    if (VEC && n == 4) {
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const float4 t = *reinterpret_cast<const float4 *>(site[i].x + r * site[i].ldx + c);
        v[i][0] = t.x, v[i][1] = t.y, v[i][2] = t.z, v[i][3] = t.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = j < n ? site[i].x[r * site[i].ldx + c + j] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      uint32_t w[4];
      dropout_words(keys[i], row0 + uint64_t(r), uint32_t(cb), w);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[i][j] = dropped(v[i][j], w[j] < threshold, inv_keep);
    }
    if (VEC && n == 4) {
#pragma unroll
      for (int i = 0; i < NS; ++i)
        *reinterpret_cast<float4 *>(site[i].out + r * site[i].ldo + c) = make_float4(v[i][0], v[i][1], v[i][2], v[i][3]);
    } else {
#pragma unroll
      for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < n) site[i].out[r * site[i].ldo + c + j] = v[i][j];
    }
  }
}

// keep bytes (1 / 0); VEC: base 4-byte aligned and ldm a multiple of four, so a whole column block is one 32-bit store
template <bool VEC, bool KD>
__global__ __launch_bounds__(TPB) void mask_kernel(int64_t rows, int32_t cols, int32_t ncb, uint8_t *mask, int64_t ldm, uint64_t key_or_site,
                                                   uint64_t row0, uint32_t threshold, const uint64_t *__restrict__ step_key) {
  const int64_t units = rows * ncb, stride = int64_t(gridDim.x) * TPB;
  const uint64_t key = site_key<KD>(key_or_site, step_key);
  for (int64_t u = int64_t(blockIdx.x) * TPB + threadIdx.x; u < units; u += stride) {
    int64_t r;
    int32_t cb;
    unit_of(u, ncb, r, cb);
    const int32_t c = cb * 4, n = cols - c < 4 ? cols - c : 4;
    uint32_t w[4];
    dropout_words(key, row0 + uint64_t(r), uint32_t(cb), w);
    uint8_t *dst = mask + r * ldm + c;
    if (VEC && n == 4) {
      const uint32_t packed = (w[0] < threshold ? 1u : 0u) | (w[1] < threshold ? 0x100u : 0u) | (w[2] < threshold ? 0x10000u : 0u) |
                              (w[3] < threshold ? 0x1000000u : 0u);      // little-endian: byte j = column c + j
      *reinterpret_cast<uint32_t *>(dst) = packed;
    } else {
      for (int j = 0; j < n; ++j) dst[j] = w[j] < threshold ? 1 : 0;
    }
  }
}

inline unsigned grid_for(int64_t units) {
  const int64_t blocks = (units + TPB - 1) / TPB;
  return unsigned(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS);
}

// what every entry checks of the block's shape; MGCN_OK, or the code with the message set
int check_block(const char *what, int64_t rows, int32_t cols) {
  MGCN_REQUIRE(rows >= 0 && cols >= 1, "%s: bad sizes (rows = %lld, cols = %d)", what, (long long)rows, cols);
  MGCN_REQUIRE(rows <= MAX_ROWS, "%s: more than 2^40 rows", what);      // (rows x column blocks: bounded by check_matrix's rows x ld)
  return MGCN_OK;
}

// a matrix of the block: non-null, ld >= cols, and rows x ld elements addressable in 64-bit arithmetic with room to spare
int check_matrix(const char *what, const char *name, const void *p, int64_t ld, int64_t rows, int32_t cols) {
  MGCN_REQUIRE(p, "%s: null pointer (%s)", what, name);
  MGCN_REQUIRE(ld >= cols, "%s: leading dimension of %s (%lld) smaller than cols = %d", what, name, (long long)ld, cols);
  MGCN_REQUIRE(ld <= (int64_t(1) << 60) / (rows > 0 ? rows : 1), "%s: rows x leading dimension of %s exceeds 2^60 elements", what, name);
  return MGCN_OK;
}

// an output may be its own input only as the same matrix: same pointer, same leading dimension
int check_alias(const char *what, const float *x, int64_t ldx, const float *out, int64_t ldo) {
  MGCN_REQUIRE(x != out || ldx == ldo, "%s: in place needs the same leading dimension (%lld, %lld)", what, (long long)ldx, (long long)ldo);
  return MGCN_OK;
}

inline bool vec_ok(const void *p, int64_t ld) { return mgcn::aligned16(p) && ld % 4 == 0; }

// the step word of the _dev entry points: one 8-byte word in device memory
int check_step_key(const char *what, const uint64_t *step_key_dev) {
  MGCN_REQUIRE(step_key_dev && (reinterpret_cast<uintptr_t>(step_key_dev) & 7u) == 0, "%s: null or misaligned pointer (step_key: one 64-bit word)", what);
  return MGCN_OK;
}

// The three entries, each in both forms. step_key_dev == nullptr: `key` arguments are keys (by value); otherwise they are site ids.
int apply_launch(const char *what, int64_t rows, int32_t cols, const float *x_dev, int64_t ldx, float *out_dev, int64_t ldo, uint64_t key,
                 const uint64_t *step_key_dev, uint64_t row0, uint32_t threshold, float inv_keep, void *stream) {
  if (int rc = check_block(what, rows, cols)) return rc;
  if (int rc = check_matrix(what, "x", x_dev, ldx, rows, cols)) return rc;
  if (int rc = check_matrix(what, "out", out_dev, ldo, rows, cols)) return rc;
  if (int rc = check_alias(what, x_dev, ldx, out_dev, ldo)) return rc;
  MGCN_REQUIRE(std::isfinite(inv_keep) && inv_keep >= 0.f, "%s: inv_keep must be a finite number >= 0", what);
  if (rows == 0) return MGCN_OK;
  const int32_t ncb = (cols + 3) / 4;
  const Site s = {x_dev, ldx, out_dev, ldo, key};
  const dim3 grid(grid_for(rows * ncb)), block(TPB);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec = vec_ok(x_dev, ldx) && vec_ok(out_dev, ldo);
  if (step_key_dev) {
    if (vec)
      apply_kernel<1, true, true><<<grid, block, 0, st>>>(rows, cols, ncb, s, s, row0, threshold, inv_keep, step_key_dev);
    else
      apply_kernel<1, false, true><<<grid, block, 0, st>>>(rows, cols, ncb, s, s, row0, threshold, inv_keep, step_key_dev);
  } else {
    if (vec)
      apply_kernel<1, true, false><<<grid, block, 0, st>>>(rows, cols, ncb, s, s, row0, threshold, inv_keep, nullptr);
    else
      apply_kernel<1, false, false><<<grid, block, 0, st>>>(rows, cols, ncb, s, s, row0, threshold, inv_keep, nullptr);
  }
  MGCN_CHECK_LAUNCH(what);
  return MGCN_OK;
}

int pair_launch(const char *what, int64_t rows, int32_t cols, const float *xa_dev, int64_t ldxa, float *outa_dev, int64_t ldoa, uint64_t key_a,
                const float *xb_dev, int64_t ldxb, float *outb_dev, int64_t ldob, uint64_t key_b, const uint64_t *step_key_dev, uint64_t row0,
                uint32_t threshold, float inv_keep, void *stream) {
  if (int rc = check_block(what, rows, cols)) return rc;
  if (int rc = check_matrix(what, "x_a", xa_dev, ldxa, rows, cols)) return rc;
  if (int rc = check_matrix(what, "out_a", outa_dev, ldoa, rows, cols)) return rc;
  if (int rc = check_matrix(what, "x_b", xb_dev, ldxb, rows, cols)) return rc;
  if (int rc = check_matrix(what, "out_b", outb_dev, ldob, rows, cols)) return rc;
  if (int rc = check_alias(what, xa_dev, ldxa, outa_dev, ldoa)) return rc;
  if (int rc = check_alias(what, xb_dev, ldxb, outb_dev, ldob)) return rc;
  MGCN_REQUIRE(outa_dev != outb_dev, "%s: the two outputs are the same matrix", what);
  // an output that is the OTHER site's input is read by the lane that writes it (reads come first), but only as the same matrix
  if (int rc = check_alias(what, xa_dev, ldxa, outb_dev, ldob)) return rc;
  if (int rc = check_alias(what, xb_dev, ldxb, outa_dev, ldoa)) return rc;
  MGCN_REQUIRE(std::isfinite(inv_keep) && inv_keep >= 0.f, "%s: inv_keep must be a finite number >= 0", what);
  if (rows == 0) return MGCN_OK;
  const int32_t ncb = (cols + 3) / 4;
  const Site a = {xa_dev, ldxa, outa_dev, ldoa, key_a}, b = {xb_dev, ldxb, outb_dev, ldob, key_b};
  const dim3 grid(grid_for(rows * ncb)), block(TPB);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec = vec_ok(xa_dev, ldxa) && vec_ok(outa_dev, ldoa) && vec_ok(xb_dev, ldxb) && vec_ok(outb_dev, ldob);
  if (step_key_dev) {
    if (vec)
      apply_kernel<2, true, true><<<grid, block, 0, st>>>(rows, cols, ncb, a, b, row0, threshold, inv_keep, step_key_dev);
    else
      apply_kernel<2, false, true><<<grid, block, 0, st>>>(rows, cols, ncb, a, b, row0, threshold, inv_keep, step_key_dev);
  } else {
    if (vec)
      apply_kernel<2, true, false><<<grid, block, 0, st>>>(rows, cols, ncb, a, b, row0, threshold, inv_keep, nullptr);
    else
      apply_kernel<2, false, false><<<grid, block, 0, st>>>(rows, cols, ncb, a, b, row0, threshold, inv_keep, nullptr);
  }
  MGCN_CHECK_LAUNCH(what);
  return MGCN_OK;
}

int mask_launch(const char *what, int64_t rows, int32_t cols, uint8_t *mask_dev, int64_t ldm, uint64_t key, const uint64_t *step_key_dev,
                uint64_t row0, uint32_t threshold, void *stream) {
  if (int rc = check_block(what, rows, cols)) return rc;
  if (int rc = check_matrix(what, "mask", mask_dev, ldm, rows, cols)) return rc;
  if (rows == 0) return MGCN_OK;
  const int32_t ncb = (cols + 3) / 4;
  const dim3 grid(grid_for(rows * ncb)), block(TPB);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec = (reinterpret_cast<uintptr_t>(mask_dev) & 3u) == 0 && ldm % 4 == 0;
  if (step_key_dev) {
    if (vec)
      mask_kernel<true, true><<<grid, block, 0, st>>>(rows, cols, ncb, mask_dev, ldm, key, row0, threshold, step_key_dev);
    else
      mask_kernel<false, true><<<grid, block, 0, st>>>(rows, cols, ncb, mask_dev, ldm, key, row0, threshold, step_key_dev);
  } else {
    if (vec)
      mask_kernel<true, false><<<grid, block, 0, st>>>(rows, cols, ncb, mask_dev, ldm, key, row0, threshold, nullptr);
    else
      mask_kernel<false, false><<<grid, block, 0, st>>>(rows, cols, ncb, mask_dev, ldm, key, row0, threshold, nullptr);
  }
  MGCN_CHECK_LAUNCH(what);
  return MGCN_OK;
}

// ------------------------------------------------------------------------------------------------
// Counter-drawn candidate lists (include/mgcn_hip.h (15)): list position (b, j) of a [B, K] block is a pure function
// of (key, global batch row row0 + b, j) and of the index, so every rank of a sharded step draws the same lists without an
// exchange. One Philox call (counter word 2 = j >> 1) serves positions 2 jp and 2 jp + 1. Integers only.
struct DrawArgs {
  int64_t n_cand, num_entities;
  const int64_t *qkey;
  int64_t num_keys;
  const int64_t *keys, *ptr;
  const int32_t *tails;
  int64_t n_tails;
  uint64_t key, row0;      // key: the list key, or the site id in mgcn_cand_draw_dev (draw_kernel forms the key from it)
  int64_t *cand;
  int64_t ldc;
  uint8_t *label;      // null: no labels, and no key lookup for the pairs that hold negatives only
  int64_t ldl;
};

// the high half of the 128-bit product: floor(r m / 2^64), a value in [0, m)
__host__ __device__ inline uint64_t mul_hi64(uint64_t r, uint64_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(r, m);
#else
  return uint64_t((static_cast<unsigned __int128>(r) * m) >> 64);
#endif
}

// The id of a negative from its 64-bit value r. NoTable: uniform, the high half of r N. AliasTable (include/mgcn_hip.h (17)): the
// high half is the slot, the upper 32 bits of the LOW half are the position inside the slot, and one 8-byte word of the table
// (alias << 32 | threshold) decides between the slot and its alias. slot < N by construction; an alias outside [0, N) is written
// as -1 and never followed.
struct NoTable {};
struct AliasTable {
  const uint64_t *word;      // [num_entities]
};

__host__ __device__ inline int64_t negative_id(uint64_t r, uint64_t n, NoTable) { return int64_t(mul_hi64(r, n)); }

__host__ __device__ inline int64_t negative_id(uint64_t r, uint64_t n, AliasTable t) {
  const uint64_t slot = mul_hi64(r, n);
  const uint32_t u = uint32_t((r * n) >> 32);
  const uint64_t w = t.word[slot];
  if (u < uint32_t(w)) return int64_t(slot);
  const uint64_t alias = w >> 32;
  return alias < n ? int64_t(alias) : int64_t(-1);
}

// Positions 2 jp and 2 jp + 1 of row b. The ONE definition: the draw kernels and the host twins all call it, T saying where a
// negative's id comes from.
template <class T>
__host__ __device__ inline void draw_pair(const DrawArgs &a, T table, int64_t b, int64_t jp) {
  uint32_t w[4];
  dropout_words(a.key, a.row0 + uint64_t(b), uint32_t(jp), w);
  const uint64_t r[2] = {uint64_t(w[0]) | uint64_t(w[1]) << 32, uint64_t(w[2]) | uint64_t(w[3]) << 32};
  // the query's run of known tails [lo, hi): mgcn_filter_mask's lookup; a run that is empty, reversed or leaves [0, n_tails] is no
  // run (lo = hi = 0), and nothing of tails is addressed through it
  int64_t lo = 0, hi = 0;
  if (a.label || jp == 0) {
    const int64_t q = a.qkey[b];
    int64_t k0 = 0, k1 = a.num_keys;
    while (k0 < k1) {
      const int64_t mid = (k0 + k1) >> 1;
      if (a.keys[mid] < q) k0 = mid + 1; else k1 = mid;
    }
    if (k0 < a.num_keys && a.keys[k0] == q) {
      const int64_t p0 = a.ptr[k0], p1 = a.ptr[k0 + 1];
      if (p0 >= 0 && p0 < p1 && p1 <= a.n_tails) lo = p0, hi = p1;
    }
  }
  for (int h = 0; h < 2; ++h) {
    const int64_t j = 2 * jp + h;
    if (j >= a.n_cand) break;
    int64_t id;
    if (j == 0)
      id = hi > lo ? int64_t(a.tails[lo + int64_t(mul_hi64(r[0], uint64_t(hi - lo)))]) : int64_t(-1);
    else
      id = negative_id(r[h], uint64_t(a.num_entities), table);
    a.cand[b * a.ldc + j] = id;
    if (a.label) {
      // the GLOBAL label, mgcn_cand_labels' for the shard [0, num_entities): the id is an entity and is found in the run
      uint8_t hit = 0;
      if (uint64_t(id) < uint64_t(a.num_entities)) {
        int64_t t0 = lo, t1 = hi;
        while (t0 < t1) {
          const int64_t mid = (t0 + t1) >> 1;
          if (int64_t(a.tails[mid]) < id) t0 = mid + 1; else t1 = mid;
        }
        hit = t0 < hi && int64_t(a.tails[t0]) == id;
      }
      a.label[b * a.ldl + j] = hit;
    }
  }
}

// KD false: a.key is the list key. KD true (mgcn_cand_draw_dev): a.key is the site id, and every thread forms the key once, ahead of
// its loop, from the step word in device memory, so a captured launch draws under the word it finds when it RUNS.
template <bool KD>
__global__ __launch_bounds__(TPB) void draw_kernel(int64_t batch, int32_t npairs, DrawArgs a, const uint64_t *__restrict__ step_key) {
  const int64_t units = batch * npairs, stride = int64_t(gridDim.x) * TPB;
  a.key = site_key<KD>(a.key, step_key);
  for (int64_t u = int64_t(blockIdx.x) * TPB + threadIdx.x; u < units; u += stride) {
    int64_t b;
    int32_t jp;
    unit_of(u, npairs, b, jp);
    draw_pair(a, NoTable(), b, jp);
  }
}

// draw_kernel with the alias table of (17): the same units, the same grid rule, one more 8-byte load per negative
template <bool KD>
__global__ __launch_bounds__(TPB) void draw_alias_kernel(int64_t batch, int32_t npairs, DrawArgs a, const uint64_t *__restrict__ table,
                                                         const uint64_t *__restrict__ step_key) {
  const int64_t units = batch * npairs, stride = int64_t(gridDim.x) * TPB;
  a.key = site_key<KD>(a.key, step_key);
  const AliasTable t = {table};
  for (int64_t u = int64_t(blockIdx.x) * TPB + threadIdx.x; u < units; u += stride) {
    int64_t b;
    int32_t jp;
    unit_of(u, npairs, b, jp);
    draw_pair(a, t, b, jp);
  }
}

// every check of mgcn_cand_draw / mgcn_cand_draw_dev / mgcn_cand_draw_host; MGCN_OK, or the code with the message set
int check_draw(const char *what, int64_t batch, const DrawArgs &a) {
  MGCN_REQUIRE(batch >= 0 && a.n_cand >= 1 && a.num_keys >= 0 && a.n_tails >= 0, "%s: bad sizes (batch = %lld, n_cand = %lld, num_keys = %lld, n_tails = %lld)",
               what, (long long)batch, (long long)a.n_cand, (long long)a.num_keys, (long long)a.n_tails);
  MGCN_REQUIRE(a.num_entities >= 1 && a.num_entities <= MAX_ROWS, "%s: num_entities = %lld outside [1, 2^40]", what, (long long)a.num_entities);
  MGCN_REQUIRE(batch < (int64_t(1) << 31) - 64 && a.n_cand < (int64_t(1) << 31) - 64, "%s: sizes exceed int32", what);
  MGCN_REQUIRE(a.qkey && a.ptr && a.cand && (a.num_keys == 0 || a.keys) && (a.n_tails == 0 || a.tails), "%s: null pointer", what);
  MGCN_REQUIRE(a.ldc >= a.n_cand && (!a.label || a.ldl >= a.n_cand), "%s: leading dimension smaller than n_cand = %lld", what, (long long)a.n_cand);
  const int64_t most = (int64_t(1) << 60) / (batch > 0 ? batch : 1);
  MGCN_REQUIRE(a.ldc <= most && (!a.label || a.ldl <= most), "%s: batch x leading dimension exceeds 2^60 elements", what);
  return MGCN_OK;
}

// what the weighted forms check on top of check_draw: the table, and a table small enough for a 31-bit alias
int check_table(const char *what, const DrawArgs &a, const int64_t *table) {
  MGCN_REQUIRE(table && mgcn::aligned8(table), "%s: null or misaligned pointer (table: num_entities 64-bit words)", what);
  MGCN_REQUIRE(a.num_entities <= (int64_t(1) << 31) - 1, "%s: num_entities = %lld above 2^31 - 1 (the alias is 31 bits)", what,
               (long long)a.num_entities);
  return MGCN_OK;
}

// the device entries: step_key_dev == nullptr: a.key is the key (by value); otherwise it is the site id. alias: the weighted forms,
// table_dev their table
int draw_launch(const char *what, int64_t batch, const DrawArgs &a, const uint64_t *step_key_dev, void *stream, bool alias = false,
                const int64_t *table_dev = nullptr) {
  if (int rc = check_draw(what, batch, a)) return rc;
  if (alias)
    if (int rc = check_table(what, a, table_dev)) return rc;
  if (batch == 0) return MGCN_OK;
  const int32_t npairs = int32_t((a.n_cand + 1) / 2);
  const dim3 grid(grid_for(batch * npairs)), block(TPB);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (alias) {
    const uint64_t *t = reinterpret_cast<const uint64_t *>(table_dev);
    if (step_key_dev)
      draw_alias_kernel<true><<<grid, block, 0, st>>>(batch, npairs, a, t, step_key_dev);
    else
      draw_alias_kernel<false><<<grid, block, 0, st>>>(batch, npairs, a, t, nullptr);
  } else if (step_key_dev)
    draw_kernel<true><<<grid, block, 0, st>>>(batch, npairs, a, step_key_dev);
  else
    draw_kernel<false><<<grid, block, 0, st>>>(batch, npairs, a, nullptr);
  MGCN_CHECK_LAUNCH(what);
  return MGCN_OK;
}

// ------------------------------------------------------------------------------------------------
// Edge dropout and own-triple removal (include/mgcn_hip.h (19)): this step's graph is a copy of the slot records with
// new norms. An undirected edge u = eid mod E is kept iff element (row u, column 0) of the site's mask is a keep bit and forced[u]
// is not set; a node's degree is the number of kept slots of its destination run in the other half (by mirror symmetry its kept
// out-degree in this one); the norm of a kept slot is T[deg(src)] * T[deg(dst)] with the host-built table T[d] = 1 / sqrt(float(d)).
// Integers and table look-ups only up to the one f32 multiply, so the copy has the feeder's bits for the kept edge list.
struct EdgeDropArgs {
  int64_t num_nodes, num_edges_half;
  const int32_t *rowptr;           // [2, N + 1]
  const mgcn_edge_rec *rec;        // [2E]
  const int32_t *slot_dst;         // [2E], bit 31 = half
  const int32_t *hubinfo, *chunks; // null: no destination is a hub
  int64_t num_chunks;
  const float *table;              // T[0 .. table_len)
  int64_t table_len;
  const uint8_t *forced;           // [E] or null
  uint64_t key;                    // the site's key, or the site id in the _dev entry point
  uint32_t threshold;
  float *cinv;                     // [2, N] workspace: T[deg_h[n]]
  mgcn_edge_rec *rec_out;          // [2E]
};

// kept(eid mod E); an edge id outside [0, 2E) is no edge and is never kept (nothing is addressed through it)
__host__ __device__ inline bool edge_kept(const EdgeDropArgs &a, int32_t eid) {
  const int64_t E = a.num_edges_half;
  if (uint64_t(int64_t(eid)) >= uint64_t(2 * E)) return false;
  const int64_t u = eid >= E ? eid - E : eid;
  uint32_t w[4];
  dropout_words(a.key, uint64_t(u), 0u, w);
  return w[0] < a.threshold && !(a.forced && a.forced[u]);
}

// the destination run [b, e) of node n in half h: the non-hub run of rowptr, or the hub's segment (its chunks are contiguous);
// whatever the arrays hold, the run stays inside [0, 2E)
__host__ __device__ inline void edge_run(const EdgeDropArgs &a, int h, int64_t n, int64_t &b, int64_t &e) {
  const int64_t N = a.num_nodes, E2 = 2 * a.num_edges_half;
  b = a.rowptr[h * (N + 1) + n], e = a.rowptr[h * (N + 1) + n + 1];
  if (a.hubinfo) {
    const int64_t first = a.hubinfo[(h * N + n) * 2], cnt = a.hubinfo[(h * N + n) * 2 + 1];
    if (cnt > 0 && first >= 0 && first + cnt <= a.num_chunks) b = a.chunks[first * 4], e = a.chunks[(first + cnt - 1) * 4 + 1];
  }
  if (b < 0) b = 0;
  if (e > E2) e = E2;
  if (e < b) e = b;
}

__host__ __device__ inline float edge_table(const EdgeDropArgs &a, int64_t deg) { return deg < a.table_len ? a.table[deg] : 0.f; }

// the new record of slot p: src, type and eid as they are, the norm of the kept graph or +0.0f
__host__ __device__ inline mgcn_edge_rec edge_record(const EdgeDropArgs &a, int64_t p) {
  mgcn_edge_rec r = a.rec[p];
  const int32_t sd = a.slot_dst[p];
  const int64_t N = a.num_nodes, n = sd & 0x7fffffff, s = r.src, h = (uint32_t(sd) >> 31) & 1u;
  float norm = 0.f;
  if (edge_kept(a, r.eid) && uint64_t(s) < uint64_t(N) && n < N) norm = a.cinv[h * N + s] * a.cinv[h * N + n];
  r.norm = norm;
  return r;
}

constexpr int EDGE_GS = 8;      // lanes per (half, node) in the degree launch

// launch 1: EDGE_GS lanes per (half h, node n) count the kept slots of n's run in half 1 - h and lane 0 stores T[count]
template <bool KD>
__global__ __launch_bounds__(TPB) void edge_degree_kernel(EdgeDropArgs a, const uint64_t *__restrict__ step_key) {
  a.key = site_key<KD>(a.key, step_key);
  const int64_t N = a.num_nodes, units = 2 * N, groups = int64_t(gridDim.x) * (TPB / EDGE_GS);
  const int lane = threadIdx.x % EDGE_GS;
  // every lane of a wave runs the same number of turns, so the shuffles below always meet whole groups
  const int64_t turns = (units + groups - 1) / groups;
  int64_t i = int64_t(blockIdx.x) * (TPB / EDGE_GS) + threadIdx.x / EDGE_GS;
  for (int64_t t = 0; t < turns; ++t, i += groups) {
    int count = 0;
    if (i < units) {
      const int h = i >= N ? 1 : 0;
      int64_t b, e;
      edge_run(a, 1 - h, i - h * N, b, e);
      for (int64_t p = b + lane; p < e; p += EDGE_GS) count += edge_kept(a, a.rec[p].eid) ? 1 : 0;
    }
#pragma unroll
    for (int m = EDGE_GS / 2; m >= 1; m >>= 1) count += __shfl_xor(count, m, EDGE_GS);
    if (i < units && lane == 0) a.cinv[i] = edge_table(a, count);
  }
}

// launch 2: one lane per slot, one 16-byte store
template <bool KD>
__global__ __launch_bounds__(TPB) void edge_records_kernel(EdgeDropArgs a, const uint64_t *__restrict__ step_key) {
  a.key = site_key<KD>(a.key, step_key);
  const int64_t slots = 2 * a.num_edges_half, stride = int64_t(gridDim.x) * TPB;
  for (int64_t p = int64_t(blockIdx.x) * TPB + threadIdx.x; p < slots; p += stride) {
    const mgcn_edge_rec r = edge_record(a, p);
    *reinterpret_cast<int4 *>(a.rec_out + p) = make_int4(r.src, r.type, __float_as_int(r.norm), r.eid);
  }
}

// every check of mgcn_edge_drop_records / _dev / _host; max_run: the longest destination run (hub segments included)
int check_edge_drop(const char *what, const EdgeDropArgs &a, int64_t max_run) {
  const int64_t N = a.num_nodes, E = a.num_edges_half;
  MGCN_REQUIRE(N >= 0 && E >= 0 && a.num_chunks >= 0 && max_run >= 0, "%s: negative size", what);
  MGCN_REQUIRE(N < (int64_t(1) << 31) - 1 && 2 * E < (int64_t(1) << 31) - 1 && a.num_chunks < (int64_t(1) << 31) - 1,
               "%s: sizes exceed int32 slots", what);
  MGCN_REQUIRE(a.rowptr && a.table && (N == 0 || a.cinv) && (E == 0 || (a.rec && a.slot_dst && a.rec_out)), "%s: null pointer", what);
  MGCN_REQUIRE(a.num_chunks == 0 || (a.hubinfo && a.chunks), "%s: null pointer (hubinfo / chunks of %lld chunks)", what, (long long)a.num_chunks);
  MGCN_REQUIRE(E == 0 || (mgcn::aligned16(a.rec) && mgcn::aligned16(a.rec_out)), "%s: records not aligned to 16 bytes", what);
  MGCN_REQUIRE(a.rec != a.rec_out, "%s: rec_out is rec (the canonical records stay as they are)", what);
  MGCN_REQUIRE(a.table_len > max_run, "%s: the table holds %lld entries, the longest run has %lld slots", what, (long long)a.table_len,
               (long long)max_run);
  return MGCN_OK;
}

int edge_drop_launch(const char *what, EdgeDropArgs a, int64_t max_run, const uint64_t *step_key_dev, void *stream) {
  if (int rc = check_edge_drop(what, a, max_run)) return rc;
  if (!a.num_chunks) a.hubinfo = a.chunks = nullptr;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.num_nodes > 0) {
    const dim3 grid(grid_for(2 * a.num_nodes * EDGE_GS)), block(TPB);
    if (step_key_dev)
      edge_degree_kernel<true><<<grid, block, 0, st>>>(a, step_key_dev);
    else
      edge_degree_kernel<false><<<grid, block, 0, st>>>(a, nullptr);
    MGCN_CHECK_LAUNCH(what);
  }
  if (a.num_edges_half > 0) {
    const dim3 grid(grid_for(2 * a.num_edges_half)), block(TPB);
    if (step_key_dev)
      edge_records_kernel<true><<<grid, block, 0, st>>>(a, step_key_dev);
    else
      edge_records_kernel<false><<<grid, block, 0, st>>>(a, nullptr);
    MGCN_CHECK_LAUNCH(what);
  }
  return MGCN_OK;
}

// One wave per query: the lower bound of its key in the sorted directed-edge keys (mgcn_filter_mask's bisection), then the lanes
// walk the run of equal keys and store byte 1 for each entry's undirected edge. Racing stores write the same value.
__global__ __launch_bounds__(TPB) void edge_flags_kernel(int32_t batch, const int64_t *__restrict__ qkey, int64_t num_edges_half,
                                                         const int64_t *__restrict__ ekeys, const int32_t *__restrict__ eund,
                                                         uint8_t *__restrict__ forced) {
  const int64_t b = int64_t(blockIdx.x) * (TPB / 64) + threadIdx.x / 64, E2 = 2 * num_edges_half;
  if (b >= batch) return;
  const int64_t q = qkey[b];
  int64_t k0 = 0, k1 = E2;
  while (k0 < k1) {
    const int64_t mid = (k0 + k1) >> 1;
    if (ekeys[mid] < q) k0 = mid + 1; else k1 = mid;
  }
  for (int64_t i = k0 + threadIdx.x % 64; i < E2 && ekeys[i] == q; i += 64) {
    const int32_t u = eund[i];
    if (uint64_t(int64_t(u)) < uint64_t(num_edges_half)) forced[u] = 1;
  }
}

}  // namespace

extern "C" int mgcn_edge_drop_records(int64_t num_nodes, int64_t num_edges_half, const int32_t *rowptr_dev, const mgcn_edge_rec *rec_dev,
                                      const int32_t *slot_dst_dev, const int32_t *hubinfo_dev, const int32_t *chunks_dev, int64_t num_chunks,
                                      const float *table_dev, int64_t table_len, int64_t max_run, const uint8_t *forced_dev, uint64_t key,
                                      uint32_t threshold, float *cinv_dev, mgcn_edge_rec *rec_out_dev, void *stream) {
  const EdgeDropArgs a = {num_nodes, num_edges_half, rowptr_dev, rec_dev,    slot_dst_dev, hubinfo_dev, chunks_dev, num_chunks,
                          table_dev, table_len,      forced_dev, key,        threshold,    cinv_dev,    rec_out_dev};
  return edge_drop_launch("mgcn_edge_drop_records", a, max_run, nullptr, stream);
}

extern "C" int mgcn_edge_drop_records_dev(int64_t num_nodes, int64_t num_edges_half, const int32_t *rowptr_dev, const mgcn_edge_rec *rec_dev,
                                          const int32_t *slot_dst_dev, const int32_t *hubinfo_dev, const int32_t *chunks_dev,
                                          int64_t num_chunks, const float *table_dev, int64_t table_len, int64_t max_run,
                                          const uint8_t *forced_dev, const uint64_t *step_key_dev, uint64_t site, uint32_t threshold,
                                          float *cinv_dev, mgcn_edge_rec *rec_out_dev, void *stream) {
  const char *what = "mgcn_edge_drop_records_dev";
  if (int rc = check_step_key(what, step_key_dev)) return rc;
  const EdgeDropArgs a = {num_nodes, num_edges_half, rowptr_dev, rec_dev,    slot_dst_dev, hubinfo_dev, chunks_dev, num_chunks,
                          table_dev, table_len,      forced_dev, site,       threshold,    cinv_dev,    rec_out_dev};
  return edge_drop_launch(what, a, max_run, step_key_dev, stream);
}

// the CPU twin, from the same inline functions; it measures the longest run itself
extern "C" int mgcn_edge_drop_records_host(int64_t num_nodes, int64_t num_edges_half, const int32_t *rowptr_host, const mgcn_edge_rec *rec_host,
                                           const int32_t *slot_dst_host, const int32_t *hubinfo_host, const int32_t *chunks_host,
                                           int64_t num_chunks, const float *table_host, int64_t table_len, const uint8_t *forced_host,
                                           uint64_t key, uint32_t threshold, float *cinv_host, mgcn_edge_rec *rec_out_host) {
  const char *what = "mgcn_edge_drop_records_host";
  EdgeDropArgs a = {num_nodes,  num_edges_half, rowptr_host, rec_host, slot_dst_host, hubinfo_host, chunks_host, num_chunks,
                    table_host, table_len,      forced_host, key,      threshold,     cinv_host,    rec_out_host};
  if (int rc = check_edge_drop(what, a, 0)) return rc;
  if (!a.num_chunks) a.hubinfo = a.chunks = nullptr;
  const int64_t N = num_nodes;
  int64_t max_run = 0;
  for (int h = 0; h < 2; ++h)
    for (int64_t n = 0; n < N; ++n) {
      int64_t b, e;
      edge_run(a, h, n, b, e);
      if (e - b > max_run) max_run = e - b;
    }
  if (int rc = check_edge_drop(what, a, max_run)) return rc;
  for (int h = 0; h < 2; ++h)
    for (int64_t n = 0; n < N; ++n) {
      int64_t b, e, count = 0;
      edge_run(a, 1 - h, n, b, e);
      for (int64_t p = b; p < e; ++p) count += edge_kept(a, rec_host[p].eid) ? 1 : 0;
      cinv_host[h * N + n] = edge_table(a, count);
    }
  for (int64_t p = 0; p < 2 * num_edges_half; ++p) rec_out_host[p] = edge_record(a, p);
  return MGCN_OK;
}

extern "C" int mgcn_edge_flags_from_queries(int32_t batch, const int64_t *qkey_dev, int64_t num_edges_half, const int64_t *ekeys_dev,
                                            const int32_t *eund_dev, uint8_t *forced_dev, void *stream) {
  const char *what = "mgcn_edge_flags_from_queries";
  MGCN_REQUIRE(batch >= 0 && num_edges_half >= 0, "%s: negative size", what);
  MGCN_REQUIRE(2 * num_edges_half < (int64_t(1) << 31) - 1, "%s: sizes exceed int32 slots", what);
  if (batch == 0 || num_edges_half == 0) return MGCN_OK;
  MGCN_REQUIRE(qkey_dev && ekeys_dev && eund_dev && forced_dev, "%s: null pointer", what);
  edge_flags_kernel<<<dim3(unsigned((int64_t(batch) + TPB / 64 - 1) / (TPB / 64))), dim3(TPB), 0, static_cast<hipStream_t>(stream)>>>(
      batch, qkey_dev, num_edges_half, ekeys_dev, eund_dev, forced_dev);
  MGCN_CHECK_LAUNCH(what);
  return MGCN_OK;
}

extern "C" int mgcn_cand_draw(int64_t batch, int64_t n_cand, int64_t num_entities, const int64_t *qkey_dev, int64_t num_keys,
                              const int64_t *keys_dev, const int64_t *ptr_dev, const int32_t *tails_dev, int64_t n_tails, uint64_t key,
                              uint64_t row0, int64_t *cand_dev, int64_t ldc, uint8_t *label_dev, int64_t ldl, void *stream) {
  const DrawArgs a = {n_cand, num_entities, qkey_dev, num_keys, keys_dev, ptr_dev, tails_dev, n_tails, key, row0, cand_dev, ldc, label_dev, ldl};
  return draw_launch("mgcn_cand_draw", batch, a, nullptr, stream);
}

extern "C" int mgcn_cand_draw_dev(int64_t batch, int64_t n_cand, int64_t num_entities, const int64_t *qkey_dev, int64_t num_keys,
                                  const int64_t *keys_dev, const int64_t *ptr_dev, const int32_t *tails_dev, int64_t n_tails,
                                  const uint64_t *step_key_dev, uint64_t site, uint64_t row0, int64_t *cand_dev, int64_t ldc,
                                  uint8_t *label_dev, int64_t ldl, void *stream) {
  const char *what = "mgcn_cand_draw_dev";
  if (int rc = check_step_key(what, step_key_dev)) return rc;
  const DrawArgs a = {n_cand, num_entities, qkey_dev, num_keys, keys_dev, ptr_dev, tails_dev, n_tails, site, row0, cand_dev, ldc, label_dev, ldl};
  return draw_launch(what, batch, a, step_key_dev, stream);
}

extern "C" int mgcn_cand_draw_host(int64_t batch, int64_t n_cand, int64_t num_entities, const int64_t *qkey_host, int64_t num_keys,
                                   const int64_t *keys_host, const int64_t *ptr_host, const int32_t *tails_host, int64_t n_tails,
                                   uint64_t key, uint64_t row0, int64_t *cand_host, int64_t ldc, uint8_t *label_host, int64_t ldl) {
  const DrawArgs a = {n_cand, num_entities, qkey_host, num_keys, keys_host, ptr_host, tails_host, n_tails, key, row0, cand_host, ldc, label_host, ldl};
  if (int rc = check_draw("mgcn_cand_draw_host", batch, a)) return rc;
  const int64_t npairs = (n_cand + 1) / 2;
  for (int64_t b = 0; b < batch; ++b)
    for (int64_t jp = 0; jp < npairs; ++jp) draw_pair(a, NoTable(), b, jp);
  return MGCN_OK;
}

extern "C" int mgcn_cand_draw_alias(int64_t batch, int64_t n_cand, int64_t num_entities, const int64_t *qkey_dev, int64_t num_keys,
                                    const int64_t *keys_dev, const int64_t *ptr_dev, const int32_t *tails_dev, int64_t n_tails,
                                    const int64_t *table_dev, uint64_t key, uint64_t row0, int64_t *cand_dev, int64_t ldc,
                                    uint8_t *label_dev, int64_t ldl, void *stream) {
  const DrawArgs a = {n_cand, num_entities, qkey_dev, num_keys, keys_dev, ptr_dev, tails_dev, n_tails, key, row0, cand_dev, ldc, label_dev, ldl};
  return draw_launch("mgcn_cand_draw_alias", batch, a, nullptr, stream, true, table_dev);
}

extern "C" int mgcn_cand_draw_alias_dev(int64_t batch, int64_t n_cand, int64_t num_entities, const int64_t *qkey_dev, int64_t num_keys,
                                        const int64_t *keys_dev, const int64_t *ptr_dev, const int32_t *tails_dev, int64_t n_tails,
                                        const int64_t *table_dev, const uint64_t *step_key_dev, uint64_t site, uint64_t row0,
                                        int64_t *cand_dev, int64_t ldc, uint8_t *label_dev, int64_t ldl, void *stream) {
  const char *what = "mgcn_cand_draw_alias_dev";
  if (int rc = check_step_key(what, step_key_dev)) return rc;
  const DrawArgs a = {n_cand, num_entities, qkey_dev, num_keys, keys_dev, ptr_dev, tails_dev, n_tails, site, row0, cand_dev, ldc, label_dev, ldl};
  return draw_launch(what, batch, a, step_key_dev, stream, true, table_dev);
}

extern "C" int mgcn_cand_draw_alias_host(int64_t batch, int64_t n_cand, int64_t num_entities, const int64_t *qkey_host, int64_t num_keys,
                                         const int64_t *keys_host, const int64_t *ptr_host, const int32_t *tails_host, int64_t n_tails,
                                         const int64_t *table_host, uint64_t key, uint64_t row0, int64_t *cand_host, int64_t ldc,
                                         uint8_t *label_host, int64_t ldl) {
  const char *what = "mgcn_cand_draw_alias_host";
  const DrawArgs a = {n_cand, num_entities, qkey_host, num_keys, keys_host, ptr_host, tails_host, n_tails, key, row0, cand_host, ldc, label_host, ldl};
  if (int rc = check_draw(what, batch, a)) return rc;
  if (int rc = check_table(what, a, table_host)) return rc;
  const AliasTable t = {reinterpret_cast<const uint64_t *>(table_host)};
  const int64_t npairs = (n_cand + 1) / 2;
  for (int64_t b = 0; b < batch; ++b)
    for (int64_t jp = 0; jp < npairs; ++jp) draw_pair(a, t, b, jp);
  return MGCN_OK;
}

extern "C" int mgcn_dropout_apply(int64_t rows, int32_t cols, const float *x_dev, int64_t ldx, float *out_dev, int64_t ldo, uint64_t key,
                                  uint64_t row0, uint32_t threshold, float inv_keep, void *stream) {
  return apply_launch("mgcn_dropout_apply", rows, cols, x_dev, ldx, out_dev, ldo, key, nullptr, row0, threshold, inv_keep, stream);
}

extern "C" int mgcn_dropout_apply_dev(int64_t rows, int32_t cols, const float *x_dev, int64_t ldx, float *out_dev, int64_t ldo,
                                      const uint64_t *step_key_dev, uint64_t site, uint64_t row0, uint32_t threshold, float inv_keep,
                                      void *stream) {
  const char *what = "mgcn_dropout_apply_dev";
  if (int rc = check_step_key(what, step_key_dev)) return rc;
  return apply_launch(what, rows, cols, x_dev, ldx, out_dev, ldo, site, step_key_dev, row0, threshold, inv_keep, stream);
}

extern "C" int mgcn_dropout_apply_pair(int64_t rows, int32_t cols, const float *xa_dev, int64_t ldxa, float *outa_dev, int64_t ldoa,
                                       uint64_t key_a, const float *xb_dev, int64_t ldxb, float *outb_dev, int64_t ldob, uint64_t key_b,
                                       uint64_t row0, uint32_t threshold, float inv_keep, void *stream) {
  return pair_launch("mgcn_dropout_apply_pair", rows, cols, xa_dev, ldxa, outa_dev, ldoa, key_a, xb_dev, ldxb, outb_dev, ldob, key_b, nullptr,
                     row0, threshold, inv_keep, stream);
}

extern "C" int mgcn_dropout_apply_pair_dev(int64_t rows, int32_t cols, const float *xa_dev, int64_t ldxa, float *outa_dev, int64_t ldoa,
                                           uint64_t site_a, const float *xb_dev, int64_t ldxb, float *outb_dev, int64_t ldob,
                                           uint64_t site_b, const uint64_t *step_key_dev, uint64_t row0, uint32_t threshold,
                                           float inv_keep, void *stream) {
  const char *what = "mgcn_dropout_apply_pair_dev";
  if (int rc = check_step_key(what, step_key_dev)) return rc;
  return pair_launch(what, rows, cols, xa_dev, ldxa, outa_dev, ldoa, site_a, xb_dev, ldxb, outb_dev, ldob, site_b, step_key_dev, row0,
                     threshold, inv_keep, stream);
}

extern "C" int mgcn_dropout_mask(int64_t rows, int32_t cols, uint8_t *mask_dev, int64_t ldm, uint64_t key, uint64_t row0,
                                 uint32_t threshold, void *stream) {
  return mask_launch("mgcn_dropout_mask", rows, cols, mask_dev, ldm, key, nullptr, row0, threshold, stream);
}

extern "C" int mgcn_dropout_mask_dev(int64_t rows, int32_t cols, uint8_t *mask_dev, int64_t ldm, const uint64_t *step_key_dev,
                                     uint64_t site, uint64_t row0, uint32_t threshold, void *stream) {
  const char *what = "mgcn_dropout_mask_dev";
  if (int rc = check_step_key(what, step_key_dev)) return rc;
  return mask_launch(what, rows, cols, mask_dev, ldm, site, step_key_dev, row0, threshold, stream);
}

extern "C" int mgcn_dropout_mask_host(int64_t rows, int32_t cols, uint8_t *mask_host, int64_t ldm, uint64_t key, uint64_t row0,
                                      uint32_t threshold) {
  const char *what = "mgcn_dropout_mask_host";
  if (int rc = check_block(what, rows, cols)) return rc;
  if (int rc = check_matrix(what, "mask", mask_host, ldm, rows, cols)) return rc;
  const int32_t ncb = (cols + 3) / 4;
  for (int64_t r = 0; r < rows; ++r)
    for (int32_t cb = 0; cb < ncb; ++cb) {
      uint32_t w[4];
      dropout_words(key, row0 + uint64_t(r), uint32_t(cb), w);
      const int32_t c = cb * 4, n = cols - c < 4 ? cols - c : 4;
      for (int j = 0; j < n; ++j) mask_host[r * ldm + c + j] = w[j] < threshold ? 1 : 0;
    }
  return MGCN_OK;
}
