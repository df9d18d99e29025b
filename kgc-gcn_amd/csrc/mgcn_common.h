// Shared by the translation units of libmgcn_hip.so (gfx950 only).
#pragma once
#include <cstdarg>
#include <cstdio>

#include "../../include/mgcn_hip.h"

namespace mgcn {

char *error_buffer();  // thread-local, 512 bytes

inline int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(error_buffer(), 512, fmt, ap);
  va_end(ap);
  return code;
}

#define MGCN_REQUIRE(cond, ...)                          \
  do {                                                   \
    if (!(cond)) return mgcn::fail(MGCN_EINVAL, __VA_ARGS__); \
  } while (0)

#define MGCN_CHECK_LAUNCH(name)                                                            \
  do {                                                                                     \
    hipError_t e_ = hipGetLastError();                                                     \
    if (e_ != hipSuccess) return mgcn::fail(MGCN_ELAUNCH, "%s: %s", name, hipGetErrorString(e_)); \
  } while (0)

// hub pre-pass (aggregate.hip): chunk sums of the hub destinations' slots -> partial_dev [num_chunks, dim]; ee16: ee_dev is a
// bf16 table (include/mgcn_hip.h (2e))
int launch_hub_partials(int64_t num_nodes, int32_t dim, int32_t num_rel_rows, const mgcn_edge_rec *rec_dev,
                        const float *x_dev, int64_t ldx, const float *rel_dev, const float *loop_rel_dev,
                        const void *ee_dev, int32_t ee_in_slot_order, int64_t ee_sub_hub, const int32_t *chunks_dev,
                        int64_t chunk_begin, int64_t chunk_end, float *partial_dev, void *stream, bool ee16 = false);

// The validated parameters of one mgcn_layer_fwd_fused call (include/mgcn_hip.h (4): the same names without _dev), filled once by
// the dispatcher (layer_fused.hip) and read by the generation it picks.
struct FusedLaunch {
  int64_t num_nodes;
  int32_t dim_in, dim_out, num_rel_rows;
  const int32_t *rowptr;
  const mgcn_edge_rec *rec;
  const float *x;
  int64_t ldx;
  const float *rel, *loop_rel;
  const void *ee;              // f32, or bf16 when ee16
  const float *loop_edge;
  const void *wp;
  const float *bias, *bn_mean, *bn_var, *bn_gamma, *bn_beta;
  float bn_eps;
  float *out;
  int64_t ldo;
  int64_t node_begin, node_end, ee_sub_in, ee_sub_out;
  const int32_t *hubinfo;      // null when the launch has no hub chunks
  int64_t chunk_begin;
  const float *partial;
  const float *rels_weight;    // null, with rel_out, when the launch does not project the relations
  float *rel_out;
  const int32_t *row_bounds;   // generation 3
  int32_t num_row_bounds;
  int32_t tune;
  uint32_t *status;            // generation 3
  void *stream;
  bool live;                   // rowptr / rec are the live view (include/mgcn_hip.h (1v)): generations 2 and 3
  bool ee16;                   // ee is a bf16 table (include/mgcn_hip.h (2e)): generations 2 and 3
};

// fused layer, lockstep generation (layer_fused2.hip): D <= 256 and O <= 208 (the shapes whose alternating layers keep
// the packed weights L2-resident only when every workgroup walks them in step)
bool fused2_takes(int32_t dim_in, int32_t dim_out);
size_t fused2_packed_bytes(int32_t dim_in, int32_t dim_out);
int fused2_pack(int32_t dim_in, int32_t dim_out, const float *w_dev, void *wp_dev, void *stream);
int fused2_launch(const FusedLaunch &a);

// fused layer, elastic generation (layer_fused3.hip): one slot walk for 256 input columns, exact-width LDS buffers, a ring of staging buffers
// coupled by LDS counters, one contiguous run of rows per workgroup
bool fused3_takes(int32_t dim_in, int32_t dim_out);
size_t fused3_packed_bytes(int32_t dim_in, int32_t dim_out);
int fused3_pack(int32_t dim_in, int32_t dim_out, const float *w_dev, void *wp_dev, void *stream);
int fused3_launch(const FusedLaunch &a);

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace mgcn
