// The host side of the layer backward (egc_amd/csrc/egc_backward_host.h) run on its own: no HIP call, no project library.
// stdin:  any number of lines (the program makes no judgement)
//           out H B basis_stride act agg_set sym_set A a_0 .. a_{A-1}  n n_src d_edges d_chunks t_edges t_chunks ws has_plan  generic no_rec rec_separate
//         ws: the caller's workspace bytes, or -1 = what egc_backward_workspace_bytes_for answers, -2 = egc_backward_workspace_bytes
// stdout: a first line "fields <name> ..." and per input line "plan <value> ...": every field of bwd_plan and of arg_plan (arg_*),
//         the instances in the notation of tests/backward_ref.py (dst, basis, src, rec).
// --instances: the rows of the lists the launches expand from: "dst fast<..>", "src src<..>", "rec sep<NS>", "arg NS".
#include <cstdio>
#include <cstring>
#include <string>

#include "egc_backward_host.h"

using namespace egc;

static std::string dst_name(int lg, int ht, int at, unsigned agg) {
  static const char* const names[] = {"sum", "mean", "max", "min", "var", "std", "symnorm"};
  std::string s = "fast<" + std::to_string(lg) + "," + std::to_string(ht) + "," + std::to_string(at);
  for (int t = 0; agg != 0 && t < at; ++t) s += std::string(t == 0 ? "," : "+") + names[(agg >> (3 * t)) & 7u];
  return s + ">";
}

static std::string src_name(int ns, unsigned fl) {
  static const struct { unsigned bit; const char* name; } bits[] = {{SRC_T, "T"}, {SRC_S, "S"}, {SRC_V, "V"}, {SRC_X, "X"}, {SRC_N, "N"},
                                                                     {SRC_XL, "XL"}, {SRC_YL, "YL"}, {SRC_REC, "REC"}};
  std::string s = "src<" + std::to_string(ns), sep = ",";
  for (const auto& b : bits)
    if (fl & b.bit) { s += sep + b.name; sep = "|"; }
  return s + ">";
}

static int instances() {
#define EGC_ROW(LG, HT, AT, ...) std::printf("dst %s\n", dst_name(LG, HT, AT, bwd_agg_pack(__VA_ARGS__)).c_str());
  EGC_BWD_DST_LISTS(EGC_ROW)
#undef EGC_ROW
#define EGC_ROW(LG, HT, AT) std::printf("dst %s\n", dst_name(LG, HT, AT, 0u).c_str());
  EGC_BWD_DST_TRIPLES(EGC_ROW)
#undef EGC_ROW
#define EGC_ROW(FL) std::printf("src %s\n", src_name(1, SRC_STATIC | (FL)).c_str());
  EGC_BWD_SRC_FLAGS(EGC_ROW)
#undef EGC_ROW
#define EGC_ROW(NS) std::printf("src %s\nrec sep<%d>\narg %d\n", src_name(NS, 0u).c_str(), NS, NS);
  EGC_BWD_NS(EGC_ROW)
#undef EGC_ROW
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--instances") == 0) return instances();
  std::printf("fields status size_status refusal ldb slots L Ls F_g W stat_k need_t has_s has_v has_x has_n table_floats extrema rule "
              "ws_tables ws_total rec rec_offset rec_entry_bytes dst basis p2 dst_lpr_log2 wpb lds_floats_per_wave dst_group_floats "
              "dst_row_blocks rec_chunk_blocks dst_grid dst_threads dst_lds rec_ns rec_group_u32 rec_blocks rec_short_rows rec_grid "
              "rec_lds src lpr_log2 src_ns src_chunk_blocks src_grid arg_status arg_lpr_log2 arg_ns arg_chunk_blocks arg_grid\n");
  egc_layer l;
  int sw[3], has_plan;
  long long n, n_src, de, dc, te, tc, ws;
  for (;;) {
    std::memset(&l, 0, sizeof(l));
    if (std::scanf("%d %d %d %d %d %d %d %d", &l.out_channels, &l.num_heads, &l.num_bases, &l.basis_stride, &l.weight_act, &l.agg_set,
                   &l.sym_set, &l.num_aggrs) != 8 || l.num_aggrs < 1 || l.num_aggrs > EGC_MAX_AGGRS || l.num_heads < 1)
      break;
    for (int t = 0; t < l.num_aggrs; ++t)
      if (std::scanf("%d", &l.aggrs[t]) != 1) return 1;
    if (std::scanf("%lld %lld %lld %lld %lld %lld %lld %d %d %d %d", &n, &n_src, &de, &dc, &te, &tc, &ws, &has_plan, &sw[0], &sw[1], &sw[2]) != 11)
      return 1;
    l.in_channels = 16;
    l.loops_all_nodes = 1;
    const BwdSwitches s = {sw[0] != 0, sw[1] != 0, sw[2] != 0};
    const BwdWorkspace w = bwd_workspace(&l, n, de, s);
    const BwdPlan p = bwd_plan(&l, BwdCounts{n, n_src, de, dc, te, tc, ws == -1 ? w.total : ws == -2 ? w.tables : (size_t)ws, has_plan != 0}, s);
    const ArgPlan a = arg_plan(p.slots, n, de, dc);
    const int P = p.Ls / 4;
    const std::string dst = p.fast ? dst_name(p.dst_lpr_log2, p.H, p.A, p.agg) : "lds/" + std::to_string(p.wpb);
    const char* basis = !p.fast ? "-" : !p.p2 ? "np2" : p.H % P == 0 ? "p2:H%P" : "p2:H<P";
    const std::string rec = p.rec_mode == BWD_REC_OFF ? "off" : p.rec_mode == BWD_REC_FUSED ? "fused" : "sep<" + std::to_string(p.rec_ns) + ">";
    std::printf("plan %d %d %s %d %d %d %d %d %d %d %d %d %d %d %d %zu %d %d %zu %zu %s %zu %u %s %s %d %d %d %d %d %d %d %u %u %zu %d %d %d %d %u "
                "%zu %s %d %d %d %u %d %d %d %d %u\n",
                p.status, p.size_status, p.refusal[0] ? p.refusal : "-", p.ldb, p.slots, p.L, p.Ls, p.F_g, p.W, p.stat_k, p.need_t,
                (int)p.has_s, (int)p.has_v, (int)p.has_x, (int)p.has_n, p.table_floats, p.ws.extrema, (int)p.ws.records, p.ws.tables,
                p.ws.total, rec.c_str(), p.rec_offset, p.rec_entry_bytes, dst.c_str(), basis, (int)p.p2, p.dst_lpr_log2, p.wpb,
                p.lds_floats_per_wave, p.dst_group_floats, p.dst_row_blocks, p.rec_chunk_blocks, p.dst_grid, p.dst_threads, p.dst_lds,
                p.rec_ns, p.rec_group_u32, p.rec_blocks, p.rec_short_rows, p.rec_grid, p.rec_lds, src_name(p.src_ns, p.src_flags).c_str(),
                p.src_lpr_log2, p.src_ns, p.src_chunk_blocks, p.src_grid, a.status, a.lpr_log2, a.ns, a.chunk_blocks, a.grid);
  }
  return 0;
}
