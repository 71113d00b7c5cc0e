// Prints the attention plans (attn_plan.h) of a token range, one line per N, for
// tests/test_attention_stream_cpu.py.  Stand-alone: any host C++17 compiler, no
// HIP, no torch.
//   attn_plan_check [route [first [last [bh]]]]     (defaults: -1 0 4097 1)
// Line: "N route q_blocks k_blocks q_block k_block k_tile q_tile k_tiles q_tiles
// stages waves lds_fwd lds_dq lds_dkv grid_fwd grid_dq grid_dkv", or "N refused".
#include <cstdio>
#include <cstdlib>

#include "attn_plan.h"

int main(int argc, char** argv) {
  const int route = argc > 1 ? std::atoi(argv[1]) : -1;
  const int first = argc > 2 ? std::atoi(argv[2]) : 0;
  const int last = argc > 3 ? std::atoi(argv[3]) : dmp::kAttnStreamMax + 1;
  const long long bh = argc > 4 ? std::atoll(argv[4]) : 1;
  for (int N = first; N <= last; ++N) {
    const dmp::AttnPlan p = dmp::plan_attention(N, route, bh);
    if (!p.ok) {
      std::printf("%d refused\n", N);
      continue;
    }
    std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %zu %zu %zu %lld %lld %lld\n", N, p.route,
                p.q_blocks, p.k_blocks, p.q_block, p.k_block, p.k_tile, p.q_tile, p.k_tiles,
                p.q_tiles, p.stages, p.waves, p.lds_fwd, p.lds_dq, p.lds_dkv, p.grid_fwd,
                p.grid_dq, p.grid_dkv);
  }
  return 0;
}
