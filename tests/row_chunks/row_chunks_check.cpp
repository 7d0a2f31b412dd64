// The index arithmetic of egc_amd/csrc/egc_row_chunks.h run on the host: no HIP call, no project library.
// stdin:  any number of CSRs, each  n_rows n_edges rowptr[0] .. rowptr[n_rows]      (the program makes no judgement)
// stdout: "chunk <ROW_CHUNK>", then per CSR "csr <index>", "slots <count>", per slot "slot <b> none" or "slot <b> <row> <s0> <s1>",
//         per row "row <r> <p0> <p1> <first> <n_part>"
#include <cstdio>
#include <vector>

#include "egc_row_chunks.h"

int main() {
  std::printf("chunk %d\n", egc::ROW_CHUNK);
  long long n_rows, n_edges;
  for (int index = 0; std::scanf("%lld %lld", &n_rows, &n_edges) == 2; ++index) {
    if (n_rows < 1) return 2;
    std::vector<int32_t> rowptr((size_t)n_rows + 1);
    for (auto& v : rowptr) {
      long long x;
      if (std::scanf("%lld", &x) != 1) return 2;
      v = (int32_t)x;
    }
    const int64_t slots = egc::chunk_slots(n_edges);
    std::printf("csr %d\nslots %lld\n", index, (long long)slots);
    for (int64_t b = 0; b < slots; ++b) {
      int64_t row, s0, s1;
      if (egc::slot_chunk(rowptr.data(), n_rows, n_edges, b, row, s0, s1))
        std::printf("slot %lld %lld %lld %lld\n", (long long)b, (long long)row, (long long)s0, (long long)s1);
      else
        std::printf("slot %lld none\n", (long long)b);
    }
    for (int64_t r = 0; r < n_rows; ++r) {
      int64_t p0, p1, first, n_part;
      egc::row_range(rowptr.data(), n_edges, r, p0, p1);
      egc::row_partials(p0, p1, first, n_part);
      std::printf("row %lld %lld %lld %lld %lld\n", (long long)r, (long long)p0, (long long)p1, (long long)first, (long long)n_part);
    }
  }
  return 0;
}
