// Layout constants of the layer-wise adaptive optimizers (optim_trust.hip,
// parallel/fused_optim.py trust_tables).  Plain C++: the bindings and the
// kernels read the same numbers.
#pragma once

namespace dmp {

// The arena is cut into chunks of at most kTrustChunk elements that never cross
// a tensor and start on a 64-element boundary; one workgroup of 256 lanes sums
// one chunk (8 float4 per lane at the full length).  A multiple of 64.
constexpr int kTrustChunk = 8192;
// Workgroups of a stage launch; more chunks than this are grid-strided.
constexpr int kTrustGridCap = 4096;
// int32 words of a chunk row (tensor id, start element, real element count) and
// of a tensor row (first chunk, chunk count, adapt flag)
constexpr int kTrustRow = 3;
// fp32 words of a tensor's result: trust (LAMB) or local lr (LARS), ||p||, and
// ||u|| (LAMB) or ||g'|| (LARS), one pad word
constexpr int kTrustOut = 4;

}  // namespace dmp
