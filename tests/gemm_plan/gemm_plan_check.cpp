// The host side of the packed basis transform (egc_amd/csrc/egc_gemm_host.h) run on its own: no HIP call, no project library.
// stdin:  any number of lines  f_in f_g w_cols flags rows                                (the program makes no judgement)
// stdout: per line  "plan f_in f_g w_cols flags valid layout ldb NV KS TB NT pack_bytes pack_bytes_max", then every launch of
//         rows x f_in (x 16-byte aligned) in the plan's family:
//           "longk status form waves tile0 tiles mult per_cu LDX R slot_bytes ring lds threads grid"   (F16X2K; a refused set of
//                                                                             launches prints "longk <status>" alone)
//           "bf16x3 status kernel ksub vec4 nt vblock0 grid_x grid_y threads pieces lds"               (BF16X3)
//         and, whatever the layout, "ranges tile_rows r0:rows ..." of the fp16x2 row walk for tile rows 64 and 16.
#include <cstdio>

#include "egc_gemm_host.h"

using namespace egc;

static void ranges(long long rows, int widest, int tile_rows) {
  std::printf("ranges %d", tile_rows);
  gemm_for_row_ranges(rows, widest, tile_rows, [&](int64_t r0, int64_t n) {
    std::printf(" %lld:%lld", (long long)r0, (long long)n);
    return (int)EGC_OK;
  });
  std::printf("\n");
}

int main() {
  static const char* const layouts[] = {"BF16X3", "F16X2", "F16X2K"};
  static const char* const forms[] = {"two_tiles", "roles", "all_in_one"};
  int f_in, f_g, w_cols, flags;
  long long rows;
  while (std::scanf("%d %d %d %d %lld", &f_in, &f_g, &w_cols, &flags, &rows) == 5) {
    const GemmPlan p = gemm_plan(f_in, f_g, w_cols, flags);
    std::printf("plan %d %d %d %d %d %s %d %d %d %d %d %zu %zu\n", f_in, f_g, w_cols, flags, (int)p.valid, layouts[p.layout], p.ldb,
                p.NV, p.KS, p.TB, p.NT, p.pack_bytes[p.layout], p.pack_bytes_max);
    if (!p.valid) continue;
    if (p.layout == GEMM_F16X2K) {
      const auto ls = gemm_longk_launches(f_in, p.NT);
      int n_tiles = 0;
      const int st = gemm_row_tiles(rows, KROWS, n_tiles);
      if (ls.status != EGC_OK || st != EGC_OK) std::printf("longk %d\n", ls.status != EGC_OK ? ls.status : st);
      for (int l = 0; ls.status == EGC_OK && st == EGC_OK && l < ls.n; ++l) {
        const GemmLongKLaunch& g = ls.l[l];
        std::printf("longk %d %s %d %d %d %d %d %d %d %d %d %zu %d %d\n", g.status, forms[g.form], g.waves, g.tile0, g.tiles, g.mult,
                    g.per_cu, g.LDX, g.R, g.slot_bytes, g.ring, g.lds, g.threads, gemm_grid(g.per_cu, n_tiles));
      }
    } else if (p.layout == GEMM_BF16X3) {
      const auto ls = gemm_bf16x3_launches(rows, f_in, p.NV, f_in % 4 == 0);
      if (ls.status != EGC_OK) std::printf("bf16x3 %d\n", ls.status);
      for (int l = 0; l < ls.n; ++l) {
        const GemmBf16x3Launch& g = ls.l[l];
        std::printf("bf16x3 %d %s %d %d %d %d %u %u %d %d %zu\n", ls.status, g.ksub > 0 ? "ws" : "staged", g.ksub, (int)g.vec4,
                    g.nt, g.vblock0, g.grid_x, g.grid_y, g.threads, g.pieces, g.lds);
      }
    }
    const int widest = std::max(std::max(f_in, p.ldb), w_cols);
    ranges(rows, widest, 64);
    ranges(rows, widest, 16);
  }
  return 0;
}
