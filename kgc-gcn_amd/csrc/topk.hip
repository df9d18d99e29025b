// Filtered top-k link prediction (section (7) of mgcn_hip.h) for gfx950.
//
// mgcn_score_topk scores an entity shard in chunks of up to TK_CHUNK rows into the caller's workspace with the launch of
// mgcn_score_fwd (so every score is that entry point's f32 value, bit for bit), then
//   topk_kernel<SELECT>  one workgroup per (query, TK_SEG-column segment of the chunk): the segment's unfiltered scores go
//                        into LDS as (key, id) pairs, a radix select keeps the k best, a bitonic sort orders them;
//   topk_kernel<MERGE>   one workgroup per query: the same selection over the segments' lists and the running list of the
//                        chunks before (also mgcn_topk_merge, the shard merge of dist.sharded_topk).
// Order: a score maps to a 32-bit key that is monotone in the f32 value (-0 and +0 share one key); a candidate ranks by
// the 64-bit word (key << 32) | ~id, so a higher score and, among equal scores, a LOWER global id comes first. The word
// is unique per entity, so the selected set and its order depend on nothing but the scores: not on the segment or chunk
// geometry, the order in which lanes append to LDS (integer LDS atomics), or the sharding.
#include <hip/hip_runtime.h>

#include <cmath>

#include "mgcn_common.h"

namespace {

constexpr int TK_THREADS = 512;                   // 8 waves
constexpr int TK_CAP = 8192;                      // candidates a workgroup holds in LDS (64 KiB of keys + ids)
constexpr int TK_KMAX = 1024;
constexpr int TK_SEG = 4096;                      // score columns per SELECT workgroup (one fill of the LDS)
constexpr int64_t TK_CHUNK = int64_t(1) << 18;    // entity rows scored per pass into the workspace

struct TopkArgs {
  // SELECT: row b of the chunk's score block [batch, lds], columns [seg * TK_SEG, min(+TK_SEG, ncols))
  const float *score;
  int64_t lds, ncols;
  int64_t id0;            // global id of chunk column 0
  const uint32_t *mask;   // filter bits of the shard (NULL: none); column j of the chunk is bit mask0 + j
  int64_t ldm, mask0;
  // MERGE: n_in candidates per row; id < 0 = padding
  const float *in_score;
  const int64_t *in_id;
  int64_t ld_in, n_in;
  // the workgroup's sorted list of k: row b at out + b * ld, SELECT list s at column (out_seg_stride * s)
  float *out_score;
  int64_t *out_id;
  int64_t ldo, ldi, out_seg_stride;
  int k;
};

struct TopkShared {
  uint32_t key[TK_CAP], id[TK_CAP];   // the candidates: [0, count)
  uint32_t okey[TK_KMAX], oid[TK_KMAX];
  uint32_t hist[256];
  uint32_t count, ocount, digit, above, bin;
};

// Order-preserving key of an f32 score: a bijection of the bit patterns (-0 folded onto +0 first) onto an unsigned order
// that is IEEE totalOrder, so NaNs with the sign bit clear rank above +inf, NaNs with it set below -inf, by bit pattern.
// Every value of the key is a candidate's (0 is the NaN 0xffffffff): "no candidate" is carried beside the key.
__device__ __forceinline__ uint32_t score_key(float s) {
  uint32_t u = __float_as_uint(s);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float key_score(uint32_t key) {
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

__device__ __forceinline__ uint64_t order_word(uint32_t key, uint32_t id) { return (uint64_t(key) << 32) | uint32_t(~id); }

// Append this lane's element (pred) at *counter: one LDS atomic per wave, slots in lane order after the wave's base.
// Every lane of the wave calls it.
__device__ __forceinline__ uint32_t wave_append(bool pred, uint32_t *counter) {
  const unsigned long long m = __ballot(pred);
  if (m == 0ull) return 0u;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll(static_cast<unsigned long long>(m)) - 1;
  uint32_t base = 0u;
  if (lane == leader) base = atomicAdd(counter, uint32_t(__popcll(m)));
  base = __shfl(base, leader);
  return base + uint32_t(__popcll(m & ((1ull << lane) - 1ull)));
}

// Keep the k best of the n > k candidates in sh.key / sh.id: afterwards they are [0, k), in no particular order.
// Radix select over the 64-bit order word, 8 bits per pass, best digits first; it stops as soon as the digit that holds
// the k-th best holds exactly the candidates still needed (for distinct scores within the first 2-4 passes; the id bits
// are only walked for ties at the threshold). Then every candidate whose word prefix is >= the threshold's is taken.
__device__ void keep_best(TopkShared &sh, int n, int k) {
  const int tid = threadIdx.x;
  uint64_t prefix = 0, pmask = 0;
  uint32_t need = uint32_t(k);
  if (tid == 0) sh.ocount = 0u;
  for (int shift = 56; shift >= 0; shift -= 8) {
    for (int i = tid; i < 256; i += TK_THREADS) sh.hist[i] = 0u;
    __syncthreads();
    for (int i = tid; i < n; i += TK_THREADS) {
      const uint64_t w = order_word(sh.key[i], sh.id[i]);
      if ((w & pmask) == prefix) atomicAdd(&sh.hist[uint32_t(w >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {   // wave 0: lane l holds digits 255 - 4l .. 252 - 4l (best first); scan the counts best first
      uint32_t c[4], s = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        c[j] = sh.hist[255 - 4 * tid - j];
        s += c[j];
      }
      uint32_t incl = s;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = __shfl_up(incl, d);
        if (tid >= d) incl += v;
      }
      uint32_t ex = incl - s;
      if (ex < need && need <= incl) {   // exactly one lane: its digits hold the need-th best
        for (int j = 0; j < 4; ++j) {
          if (need <= ex + c[j]) {
            sh.digit = uint32_t(255 - 4 * tid - j);
            sh.above = ex;
            sh.bin = c[j];
            break;
          }
          ex += c[j];
        }
      }
    }
    __syncthreads();
    const uint32_t digit = sh.digit, above = sh.above, bin = sh.bin;
    need -= above;
    prefix |= uint64_t(digit) << shift;
    pmask |= uint64_t(255) << shift;
    if (bin == need) break;   // block-uniform (read from LDS after the barrier)
  }
  // exactly k candidates have (word & pmask) >= prefix (the words are distinct); the clamp only guards a caller's
  // duplicate (score, id) entries in a merge
  for (int base = 0; base < n; base += TK_THREADS) {
    const int i = base + tid;
    uint32_t kk = 0u, ii = 0u;
    bool take = false;
    if (i < n) {
      kk = sh.key[i];
      ii = sh.id[i];
      take = (order_word(kk, ii) & pmask) >= prefix;
    }
    const uint32_t slot = wave_append(take, &sh.ocount);
    if (take && slot < uint32_t(k)) {
      sh.okey[slot] = kk;
      sh.oid[slot] = ii;
    }
  }
  __syncthreads();
  for (int i = tid; i < k; i += TK_THREADS) {
    sh.key[i] = sh.okey[i];
    sh.id[i] = sh.oid[i];
  }
  __syncthreads();
}

template <bool MERGE>
__global__ __launch_bounds__(TK_THREADS) void topk_kernel(TopkArgs p) {
  __shared__ TopkShared sh;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int k = p.k;
  const int64_t begin = MERGE ? 0 : int64_t(blockIdx.y) * TK_SEG;   // SELECT: the segment's first column
  const int64_t total = MERGE ? p.n_in : (p.ncols - begin < TK_SEG ? p.ncols - begin : TK_SEG);
  if (tid == 0) sh.count = 0u;
  __syncthreads();
  int count = 0;
  if (!MERGE) {   // a segment is one fill: all its loads first, then the appends
    constexpr int PER = TK_SEG / TK_THREADS;
    uint32_t key[PER], live = 0u;   // bit r of live: column r of this thread is an unfiltered candidate
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const int64_t j = begin + r * TK_THREADS + tid;
      key[r] = 0u;
      if (j < begin + total) {
        bool filtered = false;
        if (p.mask) {
          const int64_t m = p.mask0 + j;
          filtered = (p.mask[b * p.ldm + (m >> 5)] >> (m & 31)) & 1u;
        }
        if (!filtered) {
          key[r] = score_key(p.score[b * p.lds + j]);
          live |= 1u << r;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const bool has = (live >> r) & 1u;
      const uint32_t slot = wave_append(has, &sh.count);
      if (has) {
        sh.key[slot] = key[r];
        sh.id[slot] = uint32_t(p.id0 + begin + r * TK_THREADS + tid);
      }
    }
    __syncthreads();
    count = int(sh.count);
    if (count > k) {
      keep_best(sh, count, k);
      count = k;
    }
  } else for (int64_t pos = 0;;) {
    // MERGE, in windows: append the next candidates after the `count` held (padding entries are dropped), keep the k best
    const int take = int(TK_CAP - count < total - pos ? TK_CAP - count : total - pos);
    for (int base = 0; base < take; base += TK_THREADS) {
      const int i = base + tid;
      uint32_t key = 0u, id = 0u;
      bool has = false;
      if (i < take) {
        const int64_t j = pos + i;
        const int64_t gid = p.in_id[b * p.ld_in + j];
        if (gid >= 0) {
          key = score_key(p.in_score[b * p.ld_in + j]);
          id = uint32_t(gid);
          has = true;
        }
      }
      const uint32_t slot = wave_append(has, &sh.count);
      if (has) {
        sh.key[slot] = key;
        sh.id[slot] = id;
      }
    }
    pos += take;
    __syncthreads();
    count = int(sh.count);
    __syncthreads();   // every thread has read the counter before the next fill moves it
    if (count > k) {
      keep_best(sh, count, k);
      count = k;
      if (tid == 0) sh.count = uint32_t(k);
      __syncthreads();
    }
    if (pos >= total) break;
  }

  // order the count <= k survivors: bitonic sort of P = 2^ceil(log2 k) words, best first; padding (key 0, id ~0: word 0)
  // sorts last (a candidate's id is below 2^31, so its word is never 0)
  int P = 1;
  while (P < k) P <<= 1;
  for (int i = tid; i < P; i += TK_THREADS) {
    sh.okey[i] = i < count ? sh.key[i] : 0u;
    sh.oid[i] = i < count ? sh.id[i] : 0xffffffffu;
  }
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < P / 2; t += TK_THREADS) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const uint32_t ki = sh.okey[i], ii = sh.oid[i], kj = sh.okey[j], ij = sh.oid[j];
        const bool best_first = (i & size) == 0;
        if ((order_word(ki, ii) < order_word(kj, ij)) == best_first) {
          sh.okey[i] = kj; sh.oid[i] = ij;
          sh.okey[j] = ki; sh.oid[j] = ii;
        }
      }
      __syncthreads();
    }
  }
  const int64_t col = MERGE ? 0 : int64_t(blockIdx.y) * p.out_seg_stride;
  float *os = p.out_score + b * p.ldo + col;
  int64_t *oi = p.out_id + b * p.ldi + col;
  for (int j = tid; j < k; j += TK_THREADS) {
    if (j < count) {
      os[j] = key_score(sh.okey[j]);
      oi[j] = int64_t(sh.oid[j]);
    } else {
      os[j] = -INFINITY;
      oi[j] = -1;
    }
  }
}

size_t align256(size_t v) { return (v + 255) & ~size_t(255); }
int64_t segments(int64_t cols) { return (cols + TK_SEG - 1) / TK_SEG; }

// Workspace of mgcn_score_topk: the chunk's score block [batch, lds] f32, then the candidate rows [batch, ldc] as f32
// scores and int64 ids (list 0 = the running result of the chunks before, lists 1.. = the segments of this chunk).
struct Layout {
  int64_t lds, ldc;
  size_t score_bytes, cand_score_bytes, cand_id_bytes;
  size_t total() const { return score_bytes + cand_score_bytes + cand_id_bytes; }
};

Layout layout(int32_t batch, int64_t n_local, int32_t k) {
  Layout l;
  const int64_t rows = n_local < TK_CHUNK ? n_local : TK_CHUNK;
  l.lds = (rows + 3) & ~int64_t(3);
  l.ldc = (segments(rows) + 1) * k;
  l.score_bytes = align256(size_t(batch) * size_t(l.lds) * sizeof(float));
  l.cand_score_bytes = align256(size_t(batch) * size_t(l.ldc) * sizeof(float));
  l.cand_id_bytes = size_t(batch) * size_t(l.ldc) * sizeof(int64_t);
  return l;
}

int launch_merge(int32_t batch, int64_t n_in, const float *in_score, const int64_t *in_id, int64_t ld_in, int32_t k,
                 float *out_score, int64_t ldo, int64_t *out_id, int64_t ldi, hipStream_t stream) {
  TopkArgs p = {};
  p.in_score = in_score; p.in_id = in_id; p.ld_in = ld_in; p.n_in = n_in;
  p.out_score = out_score; p.out_id = out_id; p.ldo = ldo; p.ldi = ldi;
  p.k = k;
  hipLaunchKernelGGL(topk_kernel<true>, dim3(unsigned(batch)), dim3(TK_THREADS), 0, stream, p);
  MGCN_CHECK_LAUNCH("topk_kernel<MERGE>");
  return MGCN_OK;
}

}  // namespace

extern "C" size_t mgcn_score_topk_workspace(int32_t batch, int64_t n_local, int32_t k) {
  if (batch < 0 || n_local < 0 || k < 1 || k > TK_KMAX) return 0;
  return layout(batch, n_local, k).total();
}

extern "C" int mgcn_score_topk(int32_t batch, int64_t n_local, int64_t ent_row0, int32_t dim, const float *x_dev,
                               int64_t ldx, const float *ent_dev, int64_t lde, const float *bias_dev,
                               const uint32_t *mask_dev, int64_t ldm, int32_t k, float *out_score_dev, int64_t ldo,
                               int64_t *out_id_dev, int64_t ldi, void *workspace_dev, size_t workspace_bytes,
                               void *stream) {
  MGCN_REQUIRE(batch >= 0 && n_local >= 0 && dim > 0 && ent_row0 >= 0, "score_topk: bad sizes");
  MGCN_REQUIRE(n_local < (int64_t(1) << 31) - 64, "score_topk: sizes exceed int32");
  MGCN_REQUIRE(ent_row0 + n_local <= int64_t(INT32_MAX), "score_topk: global entity ids must stay below 2^31");
  MGCN_REQUIRE(k >= 1 && k <= TK_KMAX, "score_topk: k = %d outside [1, %d]", k, TK_KMAX);
  MGCN_REQUIRE(x_dev && (n_local == 0 || (ent_dev && bias_dev)) && out_score_dev && out_id_dev && workspace_dev,
               "score_topk: null pointer");
  MGCN_REQUIRE(ldx >= dim && lde >= dim && ldo >= k && ldi >= k, "score_topk: leading dimension too small");
  MGCN_REQUIRE(!mask_dev || ldm >= (n_local + 31) / 32, "score_topk: mask rows too short");
  const Layout l = layout(batch, n_local, k);
  MGCN_REQUIRE(workspace_bytes >= l.total(), "score_topk: workspace of %zu bytes, needs %zu", workspace_bytes, l.total());
  MGCN_REQUIRE(mgcn::aligned16(workspace_dev), "score_topk: workspace must be 16-byte aligned");
  if (batch == 0) return MGCN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_local == 0) return launch_merge(batch, 0, nullptr, nullptr, 0, k, out_score_dev, ldo, out_id_dev, ldi, s);

  char *ws = static_cast<char *>(workspace_dev);
  float *score = reinterpret_cast<float *>(ws);
  float *cand_score = reinterpret_cast<float *>(ws + l.score_bytes);
  int64_t *cand_id = reinterpret_cast<int64_t *>(ws + l.score_bytes + l.cand_score_bytes);
  const int64_t rows_max = n_local < TK_CHUNK ? n_local : TK_CHUNK;
  for (int64_t c0 = 0; c0 < n_local; c0 += rows_max) {
    const int64_t rows = n_local - c0 < rows_max ? n_local - c0 : rows_max;
    const bool first = c0 == 0, last = c0 + rows >= n_local;
    const int64_t segs = segments(rows);
    // the scores of mgcn_score_fwd: the same launch (and arithmetic choice: a chunk of an aligned table is aligned)
    if (int rc = mgcn_score_fwd(batch, rows, dim, x_dev, ldx, ent_dev + c0 * lde, lde, bias_dev + c0, score, l.lds, stream))
      return rc;
    TopkArgs p = {};
    p.score = score; p.lds = l.lds; p.ncols = rows; p.id0 = ent_row0 + c0;
    p.mask = mask_dev; p.ldm = ldm; p.mask0 = c0;
    p.k = k;
    const bool direct = first && last && segs == 1;   // one segment is the whole answer: no merge
    if (direct) {
      p.out_score = out_score_dev; p.ldo = ldo; p.out_id = out_id_dev; p.ldi = ldi;
    } else {
      p.out_score = cand_score + k; p.ldo = l.ldc; p.out_id = cand_id + k; p.ldi = l.ldc; p.out_seg_stride = k;
    }
    hipLaunchKernelGGL(topk_kernel<false>, dim3(unsigned(batch), unsigned(segs)), dim3(TK_THREADS), 0, s, p);
    MGCN_CHECK_LAUNCH("topk_kernel<SELECT>");
    if (direct) break;
    // fold: this chunk's segment lists (+ the running list of the chunks before) -> the running list, or the result
    const float *in_s = first ? cand_score + k : cand_score;
    const int64_t *in_i = first ? cand_id + k : cand_id;
    const int64_t n_in = (segs + (first ? 0 : 1)) * k;
    const int rc = last ? launch_merge(batch, n_in, in_s, in_i, l.ldc, k, out_score_dev, ldo, out_id_dev, ldi, s)
                        : launch_merge(batch, n_in, in_s, in_i, l.ldc, k, cand_score, l.ldc, cand_id, l.ldc, s);
    if (rc) return rc;
  }
  return MGCN_OK;
}

extern "C" int mgcn_topk_merge(int32_t batch, int32_t lists, const float *in_score_dev, const int64_t *in_id_dev,
                               int64_t ld_in, int32_t k, float *out_score_dev, int64_t *out_id_dev, void *stream) {
  MGCN_REQUIRE(batch >= 0 && lists >= 0, "topk_merge: bad sizes");
  MGCN_REQUIRE(k >= 1 && k <= TK_KMAX, "topk_merge: k = %d outside [1, %d]", k, TK_KMAX);
  MGCN_REQUIRE(ld_in >= int64_t(lists) * k, "topk_merge: leading dimension too small");
  MGCN_REQUIRE(out_score_dev && out_id_dev && (lists == 0 || (in_score_dev && in_id_dev)), "topk_merge: null pointer");
  if (batch == 0) return MGCN_OK;
  return launch_merge(batch, int64_t(lists) * k, in_score_dev, in_id_dev, ld_in, k, out_score_dev, k, out_id_dev, k,
                      static_cast<hipStream_t>(stream));
}
