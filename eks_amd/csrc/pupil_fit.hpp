// Launch geometry and workspace of eks_fit_pupil (eks_fit_pupil.hip), host
// side only: tools/pupil_fit_plan_check.hip walks it without a device.
//
// Two lane mappings (k_fit_accum's pair):
//   trajectory-fastest  lane = (chunk of kPupilLaneFrames frames, trajectory),
//                       trajectory fastest: from the time-major (T, E, n, B)
//                       layout every load of a wave is one row segment of
//                       consecutive trajectories.  One partial per lane.
//   frames across a wave  block = (segment of `seg` frames, trajectory); the
//                       256 threads take consecutive frames, seg / 256 each,
//                       256 apart.  One partial per block (wave shuffle, then
//                       LDS).  For few long trajectories (config 5: B = 1).
// The switch is kPupilFramesBelowB = 16 trajectories, from the access
// geometry and not from a measurement: with float32 members a wave of the
// trajectory-fastest mapping reads 64 / B row segments of 4 B bytes per load,
// which are whole 64-byte sectors from B = 16 on; below that every load uses
// a part of each sector it touches and the wave's lanes spread over 64 / B
// chunks, while frames across a wave read one contiguous span per frame step
// (B = 1: 64 frames of E n sizeof(T) bytes back to back).
//
// Neither partition depends on B: a trajectory fitted alone and the same
// trajectory in a batch of up to kPupilFramesBelowB - 1 (or of at least
// kPupilFramesBelowB) sum the same frames in the same order.
#pragma once
#include <cstddef>
#include <cstdint>

namespace eks {

constexpr int kPupilN = 8;                  // columns (fit.PUPIL_KEYS)
constexpr int kPupilBlk = 256;              // threads per block, both mappings
constexpr long long kPupilLaneFrames = 16;  // trajectory-fastest: frames per lane
constexpr long long kPupilFramesBelowB = 16;
constexpr int kPupilPartW = 8;  // doubles per partial: count, 3 means, 3 M2, 1 unused
// frames across a wave: segments of 256 * f frames, f in 1..16, so that a
// long trajectory gives ~512 blocks: the member kernels hold 182-256 VGPRs
// (two waves per SIMD), so a CU runs two blocks at a time and 512 blocks are
// one round over the 256 CUs.  More, shorter blocks run in several rounds
// and pay the block's fixed cost (the wave and block merges, 84 shuffles per
// lane) per two frames of a lane instead of per eight.
constexpr long long kPupilTargetBlocks = 512;
constexpr long long kPupilMaxLaneFrames = 16;

struct PupilPlan {
  long long B = 0, T = 0;
  bool frames_map = false;  // frames across a wave
  long long seg = 0;        // frames per partial (per lane, or per block)
  long long NP = 0;         // partials per trajectory
  long long gx = 0, gy = 0; // grid of the accumulation kernel
  size_t part_bytes = 0;    // the workspace: partials [(p * kPupilPartW + k) * B + b]
  bool ok = false;          // the grid fits a launch
};

inline PupilPlan pupil_plan(long long B, long long T) {
  PupilPlan p;
  p.B = B;
  p.T = T;
  if (B <= 0 || T < 2) return p;
  p.frames_map = B < kPupilFramesBelowB;
  if (p.frames_map) {
    long long f = (T + kPupilBlk * kPupilTargetBlocks - 1) / (kPupilBlk * kPupilTargetBlocks);
    f = f < 1 ? 1 : f > kPupilMaxLaneFrames ? kPupilMaxLaneFrames : f;
    p.seg = kPupilBlk * f;
    p.NP = (T + p.seg - 1) / p.seg;
    p.gx = p.NP;
    p.gy = B;
  } else {
    p.seg = kPupilLaneFrames;
    p.NP = (T + p.seg - 1) / p.seg;
    // lanes: p * B + b, p < NP
    const long long lanes = p.NP * B;
    p.gx = (lanes + kPupilBlk - 1) / kPupilBlk;
    p.gy = 1;
  }
  p.part_bytes = (size_t)p.NP * (size_t)B * kPupilPartW * sizeof(double);
  // (k_pupil_final: one block per trajectory)
  p.ok = p.gx >= 1 && p.gx <= 0x7fffffffLL && p.gy >= 1 && p.gy <= 65535 && B <= 0x7fffffffLL;
  return p;
}

}  // namespace eks
