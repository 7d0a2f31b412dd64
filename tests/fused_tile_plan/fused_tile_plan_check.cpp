// The host side of the one-launch batch kernel (egc_amd/csrc/egc_fused_tile_host.h) run on its own: no HIP call, no project library.
// stdin:  any number of lines (the program makes no judgement)
//           H B A L Ls ldb slots W act a_0 .. a_{A-1}  f_in with_post  tcap emax  n_graphs n_nodes  no_static ft_grid
//         no_static: EGC_NO_STATIC_CFG set (1) or not (0); ft_grid: the value of EGC_FT_GRID, or "-" = unset -- the program sets the
//         environment and ft_switches() reads it, per line
// stdout: a first line "fields <name> ..." and per input line "plan <value> ...": per direction (f_: forward, b_: backward) every
//         field of the plan, ft_tile_ok's status with the image it computed (zeros where it refused before the image), the capacity
//         and the packed operand (f_: the forward's, b_: the transposed one); then the switches and the grid.
// --time N: N calls of ft_switches() + ft_plan + ft_image on the north-star layer, "calls_per_second <value>".
#include <chrono>
#include <cstdio>
#include <cstring>

#include "egc_fused_tile_host.h"

using namespace egc;

static void print_names(const char* d) {
  for (const char* n : {"form", "quantum", "max_chunks", "max_emax", "n_ct", "n_slabs", "k16", "ldbp", "w_aw", "wl_floats", "nsets", "p0", "magic0",
                        "magic1", "k2", "ok", "off_rec", "off_planes", "off_rowinv", "off_bases", "off_wt", "off_col", "off_rowptr", "off_cnt",
                        "off_dis", "csr_stride", "off_db", "off_rowinv2", "total", "cap", "pk_tw", "pk_tiles", "pk_ksteps", "pk_columns", "pk_k_rows",
                        "pk_tail_at", "pk_tail_floats", "pk_bias_at", "pk_bytes"})
    std::printf(" %s%s", d, n);
}

static void print_plan(const FtPlan& p, int tcap, int emax) {
  FtLds L = {};
  const int ok = ft_tile_ok(p, tcap, emax, &L);
  const FtPacked& k = p.bwd ? p.packed_t : p.packed;
  std::printf(" %d %d %d %d %d %d %d %d %d %d %d %d %u %u %d %d %d %d %d %d %d %d %d %d %d %d %d %d %zu %d %d %d %d %d %d %lld %d %d %zu", (int)p.form,
              p.quantum, p.max_chunks, p.max_emax, p.n_ct, p.n_slabs, p.k16, p.ldbp, p.w_aw, p.wl_floats, p.nsets, p.p0, p.magic0, p.magic1, p.k2,
              ok, L.off_rec, L.off_planes, L.off_rowinv, L.off_bases, L.off_wt, L.off_col, L.off_rowptr, L.off_cnt, L.off_dis, L.csr_stride,
              L.off_db, L.off_rowinv2, L.total, ft_capacity(p, emax), k.tw, k.tiles, k.ksteps, k.columns(), k.tw != 0 ? k.k_rows() : 0,
              (long long)k.tail_at(), k.tail_floats, k.bias_at, k.bytes());
}

static int time_calls(long n) {
  FtLayer l = {8, 4, 4, 16, 16, 64, 16, 128, EGC_ACT_NONE, {EGC_AGGR_SUM, EGC_AGGR_MEAN, EGC_AGGR_MAX, EGC_AGGR_SYMNORM}, 128, true};
  size_t sink = 0;
  const auto t0 = std::chrono::steady_clock::now();
  for (long i = 0; i < n; ++i) {
    l.f_in = 64 + 4 * (int)(i & 15);
    const FtSwitches sw = ft_switches();
    const FtPlan p = ft_plan(l);
    sink += ft_image(p, 96, 4096 + (int)(i & 255)).total + (size_t)sw.grid;
  }
  const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::printf("calls_per_second %.0f (checksum %zu)\n", (double)n / s, sink);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 2 && std::strcmp(argv[1], "--time") == 0) return time_calls(std::atol(argv[2]));
  std::printf("fields");
  print_names("f_");
  print_names("b_");
  std::printf(" static_cfg grid_cap grid\n");
  FtLayer l;
  int with_post, tcap, emax, no_static;
  long long n_graphs, n_nodes;
  char ft_grid_env[32];
  for (;;) {
    std::memset(&l, 0, sizeof(l));
    if (std::scanf("%d %d %d %d %d %d %d %d %d", &l.H, &l.B, &l.A, &l.L, &l.Ls, &l.ldb, &l.slots, &l.W, &l.act) != 9) break;
    if (l.A < 0 || l.A > EGC_MAX_AGGRS) return 1;
    for (int t = 0; t < l.A; ++t)
      if (std::scanf("%d", &l.aggr[t]) != 1) return 1;
    if (std::scanf("%d %d %d %d %lld %lld %d %31s", &l.f_in, &with_post, &tcap, &emax, &n_graphs, &n_nodes, &no_static, ft_grid_env) != 8) return 1;
    l.with_post = with_post != 0;
    if (no_static) setenv("EGC_NO_STATIC_CFG", "1", 1); else unsetenv("EGC_NO_STATIC_CFG");
    if (std::strcmp(ft_grid_env, "-") != 0) setenv("EGC_FT_GRID", ft_grid_env, 1); else unsetenv("EGC_FT_GRID");
    const FtSwitches sw = ft_switches();
    std::printf("plan");
    print_plan(ft_plan(l), tcap, emax);
    print_plan(ftb_plan(l), tcap, emax);
    std::printf(" %d %lld %u\n", (int)sw.static_cfg, (long long)sw.grid, ft_grid(sw, n_graphs, n_nodes));
  }
  return 0;
}
