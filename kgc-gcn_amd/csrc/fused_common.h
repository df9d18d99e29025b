// What the fused layer kernels (layer_fused2.hip, layer_fused3.hip) have in common, ONE copy each: the kernel
// arguments every generation reads, the exact bf16 split, the epilogue's arithmetic, the relation projection, the gather groups'
// row bookkeeping and the weight packing. The project's promises rest on these being the same code: generations 2 and 3 give
// bit-identical rows, every generation gives the relation projection the bits of the separate launch. Internal linkage throughout
// (each translation unit compiles its own copy; everything on the device side is inlined into the kernels).
#pragma once
#include <hip/hip_runtime.h>

#include "mgcn_common.h"

namespace mgcn {

inline int cu_count() {   // compute units of the current device, or 256 (the MI355X) when the query fails
  int cus = 256, dev = 0;
  (void)hipGetDevice(&dev);
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
  return cus;
}

}  // namespace mgcn

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// The leading kernel arguments of every generation (Args2 / Args3 extend this: the offsets are part of no ABI, but the
// order is kept so that the kernels' argument loads do not move)
struct LayerArgs {
  const int32_t *rowptr;
  const int4 *rec;
  const float *x, *rel, *loop_rel, *ee, *loop_edge;   // ee: a bf16 table rides in the same field (the EE16 kernels)
  const u32x4 *wp;        // packed weights [k-block][column tile][3][64] (8 bf16 per lane), the generation's packing kernel
  const float *bias, *bn_mean, *bn_var, *bn_gamma, *bn_beta;
  float *out;
  int64_t ldx, ldo;
  int32_t n, d, o, rel_rows;
  int32_t node0, node1;   // destinations [node0, node1) are this launch's share; out row 0 = node0
  int32_t ee_sub[2];      // slot-order per-edge table shard: row of (absolute) slot s of half h = s - ee_sub[h]
  const int2 *hubinfo;    // [2][N] (first chunk, chunk count) or null
  const float *partial;   // folded hub totals (pre-pass), row (first chunk - chunk0)
  int32_t chunk0;
  const float *rw;        // relation projection: rels_weight [D, O] (model.py:107) or null
  float *rel_out;         // [rel_rows - 1, O]
};

// ---------------------------------------------------------------------------------------------- the column cut
// A gather pass ("chunk") covers at most 128 consecutive input columns: one float4 per lane of a 32-lane group. Generations 2
// and 3 walk a mode's columns in the chunks of this table; a chunk starts on a k-block (32 columns), so every MFMA sees the
// 32 columns it always saw, in the same order, whatever the cut: rows do not depend on it.
//   col0 / ncol  first column and width of the chunk (ncol a multiple of 4, <= 128)
//   kb0 / nkb    its first k-block within the mode (col0 / 32) and its k-blocks (ceil(ncol / 32))
//   cidle        the column that lanes with 4 * lig >= ncol load (they store zeros): the chunk's last valid float4, so that no
//                lane leaves the lines its pass fetches anyway — or 0, the row's head (the legacy walk)
constexpr int FUSED_TUNE_LEGACY_CUT = 1 << 14;   // `tune` bit 14 (include/mgcn_hip.h): the legacy cut, for A/B runs
constexpr int CUT_MAXCH = 8;   // D <= 1024
struct CutTable {
  int32_t col0[CUT_MAXCH], ncol[CUT_MAXCH], kb0[CUT_MAXCH], nkb[CUT_MAXCH], cidle[CUT_MAXCH];
};
struct FusedCut {
  int nch;
  CutTable t;
};
// The table as the kernels read it: one byte per chunk in a 64-bit kernel argument, kb0 | (nkb - 1) << 5, so that the roles'
// control values come out of two scalar registers with shifts (a table in memory put a scalar load and its wait in front of every
// k-block's weight prefetch: +1 us per launch, measured). col0 = 32 kb0, ncol = min(32 nkb, d - col0); the idle lanes' column is
// the chunk's last float4 where `clamp` is set, else 0.
inline uint64_t cut_pack(const CutTable &t, int nch) {
  uint64_t w = 0;
  for (int i = 0; i < nch; ++i) w |= uint64_t(t.kb0[i] | (t.nkb[i] - 1) << 5) << (8 * i);
  return w;
}
__device__ __forceinline__ int cut_kb0(uint64_t w, int c) { return int(w >> (8 * c)) & 31; }
__device__ __forceinline__ int cut_nkb(uint64_t w, int c) { return ((int(w >> (8 * c)) >> 5) & 7) + 1; }
__device__ __forceinline__ int cut_ncol(uint64_t w, int c, int d) {
  const int n = 32 * cut_nkb(w, c), left = d - 32 * cut_kb0(w, c);
  return n < left ? n : left;
}
// The line model behind the cut: rows of d floats lie 4 d bytes apart, so a row starts at byte o of a 128-byte line for every o
// that is a multiple of gcd(4 d, 128), each as often as the others. A pass over columns [c0, c0 + n) of such a row touches the
// lines of bytes [o + 4 c0, o + 4 (c0 + n)), plus — when it has idle lanes (n < 128) — the line of the float4 they load, where
// that is none of them. Returns the lines of all chunks summed over the 128 / gcd offsets; *noff = that number of offsets.
inline int cut_lines(int d, const FusedCut &c, int *noff) {
  int g = 128;
  for (int r = (4 * d) % 128; r; ) { const int t = g % r; g = r; r = t; }
  int total = 0;
  for (int o = 0; o < 128; o += g) {
    for (int i = 0; i < c.nch; ++i) {
      const int b0 = o + 4 * c.t.col0[i], b1 = b0 + 4 * c.t.ncol[i] - 1;
      total += (b1 >> 7) - (b0 >> 7) + 1;
      const int il = (o + 4 * c.t.cidle[i]) >> 7;
      if (c.t.ncol[i] < 128 && (il < (b0 >> 7) || il > (b1 >> 7))) ++total;
    }
  }
  if (noff) *noff = 128 / g;
  return total;
}
// The cut of a d-column mode. Legacy: chunks of 128 columns, the last one short, idle lanes on column 0. Otherwise the same
// chunks with the idle lanes on their chunk's last float4, except for 128 < d <= 256 (two chunks, of which the 200-wide layer
// is the case that matters): there the boundary is the multiple of 32 columns, with neither chunk above 128, that minimises
// cut_lines; ties go to the more balanced cut, then to the wider first chunk. d = 200 (offsets 0, 32, 64, 96): 128 | 72 costs
// 4.75 + 3 lines and 96 | 104 costs 3.75 + 4 — a tie that the balance decides for 96 | 104 (24 and 26 busy lanes instead of
// 32 and 18); the legacy walk pays 8.75, its idle lanes of the second pass fetching the row's first line again.
inline FusedCut fused_cut(int d, bool legacy) {
  auto two = [&](int b) {       // chunks [0, b) and [b, d); b = d: one chunk
    FusedCut c = {};
    int col = 0;
    while (col < d) {
      const int n = (c.nch == 0 && b < d) ? b : (d - col < 128 ? d - col : 128);
      c.t.col0[c.nch] = col; c.t.ncol[c.nch] = n; c.t.kb0[c.nch] = col / 32; c.t.nkb[c.nch] = (n + 31) / 32;
      c.t.cidle[c.nch] = (legacy || b >= d) ? 0 : col + n - 4;
      col += n;
      ++c.nch;
    }
    return c;
  };
  FusedCut best = two(d < 128 ? d : 128);
  if (legacy || d <= 128 || d > 256) return best;
  int best_lines = cut_lines(d, best, nullptr), best_skew = 2 * 128 > d ? 2 * 128 - d : d - 2 * 128;
  for (int b = 96; b >= 32 && d - b <= 128; b -= 32) {
    const FusedCut c = two(b);
    const int lines = cut_lines(d, c, nullptr), skew = 2 * b > d ? 2 * b - d : d - 2 * b;
    if (lines < best_lines || (lines == best_lines && skew < best_skew)) { best = c; best_lines = lines; best_skew = skew; }
  }
  return best;
}

inline void fill_layer_args(LayerArgs &p, const mgcn::FusedLaunch &a) {
  p.rowptr = a.rowptr; p.rec = reinterpret_cast<const int4 *>(a.rec);
  p.x = a.x; p.rel = a.rel; p.loop_rel = a.loop_rel; p.ee = static_cast<const float *>(a.ee); p.loop_edge = a.loop_edge;
  p.wp = reinterpret_cast<const u32x4 *>(a.wp);
  p.bias = a.bias; p.bn_mean = a.bn_mean; p.bn_var = a.bn_var; p.bn_gamma = a.bn_gamma; p.bn_beta = a.bn_beta;
  p.out = a.out; p.ldx = a.ldx; p.ldo = a.ldo;
  p.n = int32_t(a.num_nodes); p.d = a.dim_in; p.o = a.dim_out; p.rel_rows = a.num_rel_rows;
  p.node0 = int32_t(a.node_begin); p.node1 = int32_t(a.node_end);
  p.ee_sub[0] = int32_t(a.ee_sub_in); p.ee_sub[1] = int32_t(a.ee_sub_out);
  p.hubinfo = reinterpret_cast<const int2 *>(a.hubinfo); p.partial = a.partial; p.chunk0 = int32_t(a.chunk_begin);
  p.rw = a.rel_out ? a.rels_weight : nullptr; p.rel_out = a.rel_out;
}

__device__ __forceinline__ float tanh_fast(float v) {   // exp2 + rcp, 7 VALU per value
  const float t = __builtin_amdgcn_exp2f(fabsf(v) * -2.885390081777927f);
  return copysignf((1.0f - t) * __builtin_amdgcn_rcpf(1.0f + t), v);
}

// Exact three-way split of two f32 values into bf16 pieces, packed {even, odd}: hi = bf16(v) (round to nearest even),
// mid = bf16(v - hi), lo = v - hi - mid. Each difference is exact (v - hi has at most 16 significant bits, the next
// one at most 8), so hi + mid + lo == v bit for bit for finite v. Rounding (not truncating) keeps every residual at
// most HALF an ulp of the piece above it, with either sign: the cross terms the multiply drops (mid x lo, lo x mid, lo x
// lo) are below 2^-26 |a| |w| and unbiased, where a truncating split leaves 2^-24 with the sign of the product
// (tests/test_gpu_round3.py feeds rows with 2^40 of dynamic range). A non-finite v gives NaN pieces: the output row is
// NaN where the exact-f32 path may give +-1 (documented in DESIGN.md).
__device__ __forceinline__ void split3p(float v0, float v1, uint32_t &h, uint32_t &m, uint32_t &l) {
  h = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{v0, v1}, bf16x2));            // v_cvt_pk_bf16_f32
  const float r0 = v0 - __uint_as_float(h << 16), r1 = v1 - __uint_as_float(h & 0xffff0000u);
  m = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{r0, r1}, bf16x2));
  const float s0 = r0 - __uint_as_float(m << 16), s1 = r1 - __uint_as_float(m & 0xffff0000u);
  l = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{s0, s1}, bf16x2));
}
// A lane's four values of a per-edge row. The f32 table: one 16-byte load. The bf16 table (include/mgcn_hip.h (2e)): one 8-byte
// load, each value widened exactly — the f32 whose bits are uint32(h) << 16.
template <bool EE16> struct EeElem { using type = float; };
template <> struct EeElem<true> { using type = uint16_t; };
__device__ __forceinline__ float4 load_ee4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float4 load_ee4(const uint16_t *p) {
  const uint2 h = *reinterpret_cast<const uint2 *>(p);
  return make_float4(__uint_as_float(h.x << 16), __uint_as_float(h.x & 0xffff0000u), __uint_as_float(h.y << 16),
                     __uint_as_float(h.y & 0xffff0000u));
}
__device__ __forceinline__ float4 f4mul(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 f4axpy(float4 s, float4 m, float w) {
  return make_float4(s.x + m.x * w, s.y + m.y * w, s.z + m.z * w, s.w + m.w * w);
}

// ---------------------------------------------------------------------------------------------- once per workgroup
// Column c of the epilogue's per-column vectors [scale | shift] x op (op = the padded output width): model.py:103-106 as one fma,
// tanh(acc * scale + shift)
__device__ __forceinline__ void epilogue_table_entry(const LayerArgs &p, float bn_eps, float *epi, int op, int c) {
  const bool in = c < p.o;
  const float inv = in ? __builtin_amdgcn_rsqf(p.bn_var[c] + bn_eps) * p.bn_gamma[c] : 0.f;
  constexpr float third = 1.0f / 3.0f;   // (sum of the three modes) / 3, model.py:103, as a multiplication (<= 1 ulp)
  epi[c] = inv * third;
  epi[op + c] = in ? ((p.bias ? p.bias[c] : 0.f) - p.bn_mean[c]) * inv + p.bn_beta[c] : 0.f;
}
// The relation table [rel_rows - 1][D] into LDS (when it fits: a third of the gather's row loads), by waves 0 .. nwaves - 1
// (the kernel's MFMA waves)
__device__ __forceinline__ void copy_rel_table(const LayerArgs &p, float *rel_lds, int wave, int lane, int nwaves) {
  const int n4 = ((p.rel_rows - 1) * p.d) >> 2;
  for (int i = wave * 64 + lane; i < n4; i += nwaves * 64)
    reinterpret_cast<float4 *>(rel_lds)[i] = reinterpret_cast<const float4 *>(p.rel)[i];
}

// ---------------------------------------------------------------------------------------------- gather groups
// A gather group is 32 lanes (half a wave), lig the lane's index in it. Lane l of a group holds the tile's row pointers l, l + 32,
// l + 64 (clamped to the tile and to the row range). What the kernels do with them (rp_get, partition, rec_chunk) stays in each
// kernel: as functions here those change the code the compiler emits.
struct RowPtrs { int a, b, c; };
// rp: one mode's row pointers; the tile is rows [row0, row0 + h) of a range that ends at row_end
__device__ __forceinline__ RowPtrs rp_load(const int32_t *rp, int row0, int h, int row_end, int lig) {
  auto at = [&](int i) {
    int node = row0 + (i < h ? i : h);
    node = node < row_end ? node : row_end;
    return rp[node];
  };
  RowPtrs r;
  r.a = at(lig); r.b = at(lig + 32); r.c = at(lig + 64);
  return r;
}

// ---------------------------------------------------------------------------------------------- relation projection
// all_rel = rel @ rels_weight (model.py:107), by the waves that are done gathering: waves wave0 .. wave0 + nwaves - 1 of workgroup
// bid of nblk.
// One item = one relation row x 16 columns per wave: the four 16-lane groups run the four K quarters of small_matmul_kernel's
// arithmetic (sequential fmaf chains), the partial sums are added in quarter order — values bit-identical to the separate
// launch, one load round trip per 32 k.
__device__ __forceinline__ void rel_projection(const LayerArgs &p, int wave, int wave0, int nwaves, int lane, int bid, int nblk) {
  const int rows = p.rel_rows - 1, k = p.d, n = p.o;
  const int ncg = (n + 15) / 16, items = rows * ncg;
  const int kper = (k + 3) / 4;
  const int qd = lane >> 4;
  const int k0 = qd * kper, k1 = (k0 + kper < k) ? k0 + kper : k;
  for (int item = (wave - wave0) * nblk + bid; item < items; item += nblk * nwaves) {
    const int row = item / ncg, col = (item - row * ncg) * 16 + (lane & 15);
    const bool ok = col < n;
    const float *ap = p.rel + int64_t(row) * k;
    const float *bp = p.rw + (ok ? col : 0);
    float a = 0.f;
    constexpr int UR = 32;
    for (int i0 = 0; i0 < kper; i0 += UR) {
      float av[UR], bv[UR];
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        const int kk = k0 + i0 + u;
        const int kc = (i0 + u < kper && kk < k1) ? kk : 0;
        av[u] = ap[kc];
        bv[u] = bp[int64_t(kc) * n];
      }
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        const int kk = k0 + i0 + u;
        if (i0 + u < kper && kk < k1) a = fmaf(av[u], bv[u], a);
      }
    }
    const float q1 = __shfl(a, (lane & 15) + 16), q2 = __shfl(a, (lane & 15) + 32), q3 = __shfl(a, (lane & 15) + 48);
    if (qd == 0 && ok) p.rel_out[int64_t(row) * n + col] = ((a + q1) + q2) + q3;
  }
}

// ---------------------------------------------------------------------------------------------- weight packing
// Thread idx of a packing kernel writes wp[idx], idx = ((g * nt + ct) * 3 + piece) * 64 + lane: piece `piece` of the exact split
// of the 8 values at(g, 8 * (lane >> 4) + i, 16 * ct + (lane & 15)), i = 0..7 — row 0..31 of k-block g, output column.
template <class At>
__device__ __forceinline__ void pack_lane(u32x4 *wp, int idx, int nt, At at) {
  const int lane = idx & 63, piece = (idx >> 6) % 3, ct = ((idx >> 6) / 3) % nt, g = (idx >> 6) / (3 * nt);
  const int col = ct * 16 + (lane & 15), k0 = 8 * (lane >> 4);
  uint32_t bits[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float v[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) v[j] = at(g, k0 + 2 * i + j, col);
    uint32_t h, m, l;
    split3p(v[0], v[1], h, m, l);
    bits[i] = piece == 0 ? h : piece == 1 ? m : l;
  }
  wp[idx] = u32x4{bits[0], bits[1], bits[2], bits[3]};
}

// Generations 2 and 3: wp[((g * NT + ct) * 3 + piece) * 64 + lane] = 8 bf16: W[mode * D + 32 kbi + 8 (lane >> 4) + i]
// [16 ct + (lane & 15)], i = 0..7, zero outside; g = mode * kbm + kbi (k-block kbi of the mode: 32 consecutive input columns,
// kbm = ceil(D / 32) of them). The two generations differ in the number of column tiles only: for O > 128 they share the packing.
struct ModeWeights {
  const float *w;
  int d, o, kbm;
  __device__ __forceinline__ float operator()(int g, int kl, int col) const {
    const int mode = g / kbm, k = 32 * (g - mode * kbm) + kl;
    return (k < d && col < o) ? w[(int64_t(mode) * d + k) * o + col] : 0.f;
  }
};
inline int pack_modes_kbm(int d) { return (d + 31) / 32; }
inline size_t pack_modes_bytes(int d, int nt) { return size_t(3 * pack_modes_kbm(d)) * nt * 3 * 64 * 16; }

// The packing kernel over kblocks k-blocks x nt column tiles (templates: only the translation units that pack this way emit it)
template <class At>
__global__ __launch_bounds__(256) void pack_kernel(u32x4 *__restrict__ wp, int nt, int total, At at) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < total) pack_lane(wp, idx, nt, at);
}
template <class At>
int pack_launch(void *wp_dev, int kblocks, int nt, At at, void *stream) {
  const int total = kblocks * nt * 3 * 64;
  hipLaunchKernelGGL(pack_kernel<At>, dim3(unsigned((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<u32x4 *>(wp_dev), nt, total, at);
  MGCN_CHECK_LAUNCH("pack_kernel");
  return MGCN_OK;
}

}  // namespace
