// The WIDE instances of the one-launch batch kernel (egc_fused_tile_dev.h): the reference's own batched layer shapes beyond
// d = 128 -- zinc / cifar EGC-S 168 / H8 / B4, molhiv EGC-S 296 / H8 / B4 and EGC-M 224 / H4 / B4 (run_pretrained.sh:7,12,23,24;
// hyperparameters.md) -- i.e. layers.py:97-101,110 with F_in up to 320 and up to 384 columns of [bases | weightings]:
// 32-row chunks on v_mfma_f32_32x32x16_f16, weight fragments streamed from L2, x staged in k-slabs of 128.  Included by
// egc_fused_tile_wide{1,2,3}.hip with EGC_FTW_NS = the number of k-slabs per chunk (ceil(F_in / 128): a template parameter of
// the kernel) -- translation units of their own so that the instances compile side by side.
#include <stdlib.h>

#include "egc_fused_tile_dev.h"

#define EGC_FTW_CAT_(a, b) a##b
#define EGC_FTW_CAT(a, b) EGC_FTW_CAT_(a, b)

namespace egc {

template <int LPR_LOG2, int HPB, int NEED, class C>
static int launch_ftw_one(const AggArgs& a, const FusedTileArgs& t, unsigned grid, size_t lds, hipStream_t stream) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&fused_tile_kernel<LPR_LOG2, HPB, NEED, C, EGC_FTW_NS>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) { set_last_error("hipFuncSetAttribute(fused_tile_kernel, wide)", e); return EGC_ERR_HIP; }
    attr_set = true;
  }
  fused_tile_kernel<LPR_LOG2, HPB, NEED, C, EGC_FTW_NS><<<grid, FT_THREADS, lds, stream>>>(a, t);
  EGC_LAUNCH_CHECK("fused_tile_kernel (wide)");
  return EGC_OK;
}

template <int LPR_LOG2>
static int launch_ftw_rt(const AggArgs& a, const FusedTileArgs& t, int need, unsigned grid, size_t lds, hipStream_t stream) {
  const int hpb = (a.H + a.B - 1) / a.B;
  if (need == 0) {
    if (hpb <= 1) return launch_ftw_one<LPR_LOG2, 1, 0, RtCfg>(a, t, grid, lds, stream);
    if (hpb <= 2) return launch_ftw_one<LPR_LOG2, 2, 0, RtCfg>(a, t, grid, lds, stream);
    return launch_ftw_one<LPR_LOG2, 4, 0, RtCfg>(a, t, grid, lds, stream);
  }
  if (hpb <= 1) return launch_ftw_one<LPR_LOG2, 1, NEED_SQ | NEED_MN, RtCfg>(a, t, grid, lds, stream);
  if (hpb <= 2) return launch_ftw_one<LPR_LOG2, 2, NEED_SQ | NEED_MN, RtCfg>(a, t, grid, lds, stream);
  return launch_ftw_one<LPR_LOG2, 4, NEED_SQ | NEED_MN, RtCfg>(a, t, grid, lds, stream);
}

int EGC_FTW_CAT(launch_fused_tile_wide, EGC_FTW_NS)(const AggArgs& a, const FusedTileArgs& t, int lpr, int need, unsigned grid, size_t lds, hipStream_t stream) {
  // the reference's own batched nets (run_pretrained.sh:7,12,23,24; EfficientGraphConv: symadd looped, the others raw), with
  // every layer constant compiled in: the rows phase is bound by the vector instructions of a row turn
  // (a layer without a symnorm aggregator never reads the looped set's extras: EGConv(add_self_loops=False) with the same
  // aggregators -- sym_set RAW -- computes the same numbers through the same instance)
  bool has_sym = false;
  for (int k = 0; k < a.A; ++k) has_sym |= a.aggr[k] == EGC_AGGR_SYMNORM;
  if (getenv("EGC_NO_STATIC_CFG") == nullptr && a.act == EGC_ACT_NONE && !a.x_looped && ((a.y_looped && a.loops_all) || !has_sym)) {
    constexpr int S = EGC_AGGR_SUM, M = EGC_AGGR_MEAN, X = EGC_AGGR_MAX, Y = EGC_AGGR_SYMNORM;
    unsigned pk = 0;
    for (int k = 0; k < a.A; ++k) pk |= (unsigned)a.aggr[k] << (3 * k);
    (void)S; (void)M; (void)X; (void)Y; (void)pk;
#if EGC_FTW_NS == 2
    if (a.H == 8 && a.B == 4 && a.L == 21 && a.Ls == 24 && a.A == 1 && pk == agg_pack(Y))         // zinc / cifar EGC-S 168 / H8 / B4 symadd
      return launch_ftw_one<5, 2, 0, StCfg<8, 4, 21, 1, agg_pack(Y), EGC_ACT_NONE, false, true, true, 24>>(a, t, grid, lds, stream);
    if (a.H == 4 && a.B == 4 && a.L == 56 && a.Ls == 56 && a.A == 3 && pk == agg_pack(S, M, X))   // molhiv EGC-M 224 / H4 / B4 add,mean,max
      return launch_ftw_one<6, 1, 0, StCfg<4, 4, 56, 3, agg_pack(S, M, X), EGC_ACT_NONE, false, true, true, 56>>(a, t, grid, lds, stream);
#elif EGC_FTW_NS == 3
    if (a.H == 8 && a.B == 4 && a.L == 37 && a.Ls == 40 && a.A == 1 && pk == agg_pack(Y))         // molhiv EGC-S 296 / H8 / B4 symadd
      return launch_ftw_one<6, 2, 0, StCfg<8, 4, 37, 1, agg_pack(Y), EGC_ACT_NONE, false, true, true, 40>>(a, t, grid, lds, stream);
#endif
  }
  switch (lpr) {
    case 16: return launch_ftw_rt<4>(a, t, need, grid, lds, stream);
    case 32: return launch_ftw_rt<5>(a, t, need, grid, lds, stream);
    default: return launch_ftw_rt<6>(a, t, need, grid, lds, stream);
  }
}

}  // namespace egc
