// The host side that the two attention launchers (egc_gatv2.hip, egc_gat.hip) share, each piece once: the launch geometry, the
// forward workspace, the form (S, VEC, SMALL) and its dispatch, the argument checks common to both forwards and to both
// backwards, the dropout record and the grids.  What a flavour alone knows -- its own operands' strides and pointers, its
// backward workspace, its kernels' names and arguments -- stays beside its launcher.
#pragma once
#include <initializer_list>

#include "egc_gat_dev.h"

namespace egc {

struct GatGeom {
  int32_t S, G, V;
};

static inline GatGeom gat_geom(int32_t width) {
  const int lanes = (width + 3) / 4;
  GatGeom q;
  q.S = lanes > 64 ? 2 : 1;
  int G = 1;
  while (G < lanes && G < 64) G <<= 1;
  q.G = G, q.V = q.S * G;
  return q;
}

static inline int64_t gat_blocks(int64_t groups, int32_t G) { return ceil_div(groups, 256 / G); }
static inline size_t gat_align(size_t floats) { return (floats + 3) & ~(size_t)3; }

static inline bool gat_shape_ok(int32_t H, int32_t C) { return H >= 1 && C >= 1 && (int64_t)H * C <= 512; }

// The grid of a launch with one group of G lanes per slot (a chunks launch) or per row (a rows launch).  The checks below hold
// rows and entries under 2^31 and a block has at least four groups, so the block count is a 32-bit grid dimension.
static inline unsigned gat_grid(int64_t groups, int32_t G) { return (unsigned)gat_blocks(groups, G); }

// bytes of the forward workspace: per slot and virtual lane three f4 (m, l, acc)
static inline size_t gat_fwd_ws_bytes(int64_t n_edges, int32_t H, int32_t C) {
  if (n_edges <= 0 || !gat_shape_ok(H, C)) return 0;
  return (size_t)chunk_slots(n_edges) * (size_t)gat_geom(H * C).V * 3 * 16;
}

static void gat_fill_walk(GatWalk& W, int32_t H, int32_t C, float slope, int32_t self_loops) {
  const GatGeom q = gat_geom(H * C);
  W.H = H, W.C = C, W.width = H * C, W.G = q.G, W.V = q.V, W.seg = (C + 3) / 4 + 1, W.self_loops = self_loops, W.slope = slope;
}

// the walk of a destination rows launch of which only D is wanted: no entries, no self entry
template <class Walk>
static inline Walk gat_walk_only_D(Walk W) {
  W.n_edges = 0, W.self_loops = 0;
  return W;
}

// p in (0, 1) and a seed: threshold = floor(p 2^32) and scale = 1 / (1 - p), both from p in double.  A backward that names a
// transposed CSR names its entries' forward positions too (a forward passes neither).
static inline bool gat_fill_drop(GatDrop& R, double p, const int64_t* seed, const int32_t* t_rowptr, const int32_t* t_edge_id) {
  if (!(p > 0.0 && p < 1.0) || seed == nullptr || (t_rowptr != nullptr && t_edge_id == nullptr)) return false;
  R.seed = seed, R.edge_id = t_edge_id;
  R.threshold = (uint32_t)(uint64_t)(p * 4294967296.0);
  R.scale = (float)(1.0 / (1.0 - p));
  return true;
}

// ----------------------------------------------------------------------------------------------------------- form, dispatch

// Two quads per lane above 256 columns; 16-byte accesses when the width, every stride and every pointer the call names allow
// them (NULL counts as aligned); the per-column head sums of C < 4.
struct GatForm {
  int S;
  bool vec, small;
};

static inline GatForm gat_form(int32_t H, int32_t C, std::initializer_list<int32_t> strides, std::initializer_list<const void*> pointers) {
  GatForm f = {gat_geom(H * C).S, all_mult4(H * C), C < 4};
  for (const int32_t ld : strides) f.vec = f.vec && all_mult4(ld);
  for (const void* p : pointers) f.vec = f.vec && aligned16(p);
  return f;
}

template <int S_, bool VEC_, bool SMALL_>
struct GatTag {
  static constexpr int S = S_;
  static constexpr bool VEC = VEC_, SMALL = SMALL_;
};

// launch(GatTag<S, VEC, SMALL>{}) for the form: a launch site is a generic lambda [&](auto f) that names its kernel template as
// kernel<f.S, f.VEC, f.SMALL, ...>, the plain instance or the DROP one (the tag is an empty value: its members are constants)
template <class Launch>
static inline void gat_dispatch(const GatForm& f, Launch&& launch) {
  if (f.S == 2) {
    if (f.vec) { if (f.small) launch(GatTag<2, true, true>{}); else launch(GatTag<2, true, false>{}); }
    else { if (f.small) launch(GatTag<2, false, true>{}); else launch(GatTag<2, false, false>{}); }
  } else {
    if (f.vec) { if (f.small) launch(GatTag<1, true, true>{}); else launch(GatTag<1, true, false>{}); }
    else { if (f.small) launch(GatTag<1, false, true>{}); else launch(GatTag<1, false, false>{}); }
  }
}

// ---------------------------------------------------------------------------------------------------------- argument checks

// An argument check's answer "launch": every other answer is the entry's return code (EGC_OK: nothing to do).
constexpr int GAT_RUN = -1;

// Both forwards, in the order the codes have always had: EGC_ERR_INVALID, then _UNSUPPORTED, then _WORKSPACE.  The flavour's own
// comparisons come in as values and take their place in that order: own_strides (its operands' strides reach their widths)
// before the nothing-to-do return, own_operands (its operands are there) after it.
static inline int gat_forward_args(const int32_t* rowptr, const int32_t* col, int64_t n_rows, int64_t n_edges, int64_t n_src_rows,
                                   int32_t H, int32_t C, int32_t self_loops, const float* xl, int32_t ld_xl, const float* out,
                                   int32_t ld_out, const float* lse, const void* workspace, size_t workspace_bytes, bool own_strides,
                                   bool own_operands) {
  if (!gat_shape_ok(H, C) || n_rows < 0 || n_edges < 0 || n_src_rows < 0) return EGC_ERR_INVALID;
  if (ld_xl < H * C || ld_out < H * C || !own_strides) return EGC_ERR_INVALID;
  if (self_loops && n_src_rows != n_rows) return EGC_ERR_INVALID;
  if (n_rows == 0) return EGC_OK;
  if (rowptr == nullptr || out == nullptr || lse == nullptr || !own_operands) return EGC_ERR_INVALID;
  if ((n_edges > 0 || self_loops) && xl == nullptr) return EGC_ERR_INVALID;
  if (n_edges > 0 && (col == nullptr || n_src_rows == 0)) return EGC_ERR_INVALID;
  if (!counts_fit_int32(n_rows, n_edges, n_src_rows)) return EGC_ERR_UNSUPPORTED;
  if (chunk_slots(n_edges) > 0 && !workspace_ok(workspace, workspace_bytes, gat_fwd_ws_bytes(n_edges, H, C))) return EGC_ERR_WORKSPACE;
  return GAT_RUN;
}

// Both backwards, likewise.  wanted: some gradient is; empty: the flavour's answer for n_rows == 0; src_pass: the transposed CSR
// is walked; ws_bytes: the flavour's egc_*_backward_workspace_bytes.
static inline int gat_backward_args(const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_col,
                                    int64_t n_rows, int64_t n_edges, int32_t H, int32_t C, const float* xl, int32_t ld_xl,
                                    const float* out, int32_t ld_out, const float* lse, const float* g, int32_t ld_g, const float* dxl,
                                    int32_t ld_dxl, const void* workspace, size_t workspace_bytes,
                                    size_t (*ws_bytes)(int64_t, int64_t, int32_t, int32_t), bool own_strides, bool wanted, int empty,
                                    bool own_operands, bool src_pass) {
  if (!gat_shape_ok(H, C) || n_rows < 0 || n_edges < 0) return EGC_ERR_INVALID;
  if (ld_xl < H * C || ld_out < H * C || ld_g < H * C || (dxl != nullptr && ld_dxl < H * C) || !own_strides) return EGC_ERR_INVALID;
  if (!wanted) return EGC_OK;
  if (n_rows == 0) return empty;
  if (rowptr == nullptr || xl == nullptr || out == nullptr || lse == nullptr || g == nullptr || !own_operands) return EGC_ERR_INVALID;
  if (n_edges > 0 && col == nullptr) return EGC_ERR_INVALID;
  if (src_pass && (t_rowptr == nullptr || (n_edges > 0 && t_col == nullptr))) return EGC_ERR_INVALID;
  if (!counts_fit_int32(n_rows, n_edges)) return EGC_ERR_UNSUPPORTED;
  if (!workspace_ok(workspace, workspace_bytes, ws_bytes(n_rows, n_edges, H, C))) return EGC_ERR_WORKSPACE;
  return GAT_RUN;
}

}  // namespace egc
