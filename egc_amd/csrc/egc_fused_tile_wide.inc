// The WIDE instances of the one-launch batch kernel (egc_fused_tile_dev.h): the reference's own batched layer shapes beyond
// d = 128 -- zinc / cifar EGC-S 168 / H8 / B4, molhiv EGC-S 296 / H8 / B4 and EGC-M 224 / H4 / B4 (run_pretrained.sh:7,12,23,24;
// hyperparameters.md) -- i.e. layers.py:97-101,110 with F_in up to 320 and up to 384 columns of [bases | weightings]:
// 32-row chunks on v_mfma_f32_32x32x16_f16, weight fragments streamed from L2, x staged in k-slabs of 128.  Included by
// egc_fused_tile_wide{1,2,3}.hip with EGC_FTW_NS = the number of k-slabs per chunk (ceil(F_in / 128): a template parameter of
// the kernel) -- translation units of their own so that the instances compile side by side.
#include "egc_aggregate_host.h"
#include "egc_fused_tile_dev.h"

#define EGC_FTW_CAT_(a, b) a##b
#define EGC_FTW_CAT(a, b) EGC_FTW_CAT_(a, b)

namespace egc {

template <int LPR_LOG2, int HPB, int NEED, class C>
static int launch_ftw_one(const AggArgs& a, const FusedTileArgs& t, unsigned grid, size_t lds, hipStream_t stream) {
  const auto kern = &fused_tile_kernel<LPR_LOG2, HPB, NEED, C, EGC_FTW_NS>;
  EGC_ALLOW_DYNAMIC_LDS(kern, 160 * 1024, "fused_tile_kernel, wide");
  kern<<<grid, FT_THREADS, lds, stream>>>(a, t);
  EGC_LAUNCH_CHECK("fused_tile_kernel (wide)");
  return EGC_OK;
}

// The reference's own batched nets (run_pretrained.sh:7,12,23,24; EfficientGraphConv: symadd looped, the others raw) run with
// every layer constant compiled in: the rows phase is bound by the vector instructions of a row turn.  A layer without a
// symnorm aggregator never reads the looped set's extras: EGConv(add_self_loops=False) with the same aggregators -- sym_set
// RAW -- computes the same numbers through the same instance, so only a layer WITH symnorm has to match the sets too.
template <class C>
static bool ftw_cfg_matches(const AggArgs& a) {
  bool has_sym = false;
  for (int k = 0; k < a.A; ++k) has_sym |= a.aggr[k] == EGC_AGGR_SYMNORM;
  return cfg_layer_matches<C>(a) && (!has_sym || cfg_matches<C>(a));
}

int EGC_FTW_CAT(launch_fused_tile_wide, EGC_FTW_NS)(const AggArgs& a, const FusedTileArgs& t, int need, const FtSwitches& sw, unsigned grid, size_t lds,
                                                    hipStream_t stream) {
  if (sw.static_cfg) {
    using namespace cfg;     // S, M, X, Y
#if EGC_FTW_NS == 2
    using ZincS = StCfg<8, 4, 21, 1, agg_pack(Y), EGC_ACT_NONE, false, true, true, 24>;          // zinc / cifar EGC-S 168 / H8 / B4 symadd
    using MolhivM = StCfg<4, 4, 56, 3, agg_pack(S, M, X), EGC_ACT_NONE, false, true, true, 56>;  // molhiv EGC-M 224 / H4 / B4 add,mean,max
    if (ftw_cfg_matches<ZincS>(a)) return launch_ftw_one<5, 2, 0, ZincS>(a, t, grid, lds, stream);
    if (ftw_cfg_matches<MolhivM>(a)) return launch_ftw_one<6, 1, 0, MolhivM>(a, t, grid, lds, stream);
#elif EGC_FTW_NS == 3
    using MolhivS = StCfg<8, 4, 37, 1, agg_pack(Y), EGC_ACT_NONE, false, true, true, 40>;        // molhiv EGC-S 296 / H8 / B4 symadd
    if (ftw_cfg_matches<MolhivS>(a)) return launch_ftw_one<6, 2, 0, MolhivS>(a, t, grid, lds, stream);
#endif
  }
  return agg_dispatch<NeedCoarse>(a, need, [&](auto lpr, auto hpb, auto nd) {
    return launch_ftw_one<decltype(lpr)::value, decltype(hpb)::value, decltype(nd)::value, RtCfg>(a, t, grid, lds, stream);
  });
}

}  // namespace egc
