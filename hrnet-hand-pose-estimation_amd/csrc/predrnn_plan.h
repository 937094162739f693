// The launch plan of hrnet_sample_stats (csrc/predrnn.hip): plain host arithmetic in a header of its own so that
// csrc/host_check/predrnn_host_check.cpp runs it under the sanitizers without a device.
//
// Up to PRS_MAPS dense maps of B samples each, n[m] elements per sample (n[m] a multiple of 4, 0 = map absent; the maps
// present come first). Sample b of map m is cut into parts[m] = ceil(n[m] / PRS_CHUNK) parts of PRS_CHUNK consecutive
// elements (the last one holds what is left); one workgroup of the first kernel owns one part. The workgroups of map m are
// first[m] .. first[m] + B parts[m] - 1, sample-major: workgroup first[m] + b parts[m] + k owns part k of sample b, and
// writes its two double partial sums to scratch[2 (first[m] + b parts[m] + k)]. The second kernel has one workgroup per
// (map, sample) and adds that sample's parts in the order k = lane, lane + 64, ... per lane and then the fixed tree over
// the lanes. A function of the shape alone, so two launches add in the same order.
#pragma once

#define PRS_MAPS 3
#define PRS_THREADS 256
#define PRS_VEC 8                                         // float4 loads per thread of the first kernel
#define PRS_CHUNK (PRS_THREADS * PRS_VEC * 4)             // elements per part: 8192

struct PrsPlan {
  long long n[PRS_MAPS];       // elements per sample
  long long first[PRS_MAPS];   // first workgroup of the map
  int parts[PRS_MAPS];         // parts per sample
  int maps, B;
  long long blocks;            // workgroups of the first kernel
  long long bytes;             // scratch: two doubles per workgroup
};

// 0 if the shape cannot be planned (an absent map in front of a present one, a size that is no multiple of 4, more
// workgroups than a grid holds)
inline int prs_plan(int B, const long long* n, PrsPlan* p) {
  if (B < 1) return 0;
  p->maps = 0;
  p->B = B;
  p->blocks = 0;
  for (int m = 0; m < PRS_MAPS; ++m) {
    p->n[m] = n[m];
    p->first[m] = p->blocks;
    p->parts[m] = 0;
    if (n[m] == 0) continue;
    if (n[m] < 0 || n[m] % 4 || m != p->maps) return 0;
    const long long parts = (n[m] + PRS_CHUNK - 1) / PRS_CHUNK;
    if (parts > 0x7fffffffLL / B) return 0;
    p->parts[m] = (int)parts;
    p->blocks += parts * B;
    if (p->blocks > 0x7fffffffLL) return 0;
    p->maps = m + 1;
  }
  if (p->maps == 0) return 0;
  p->bytes = p->blocks * 2 * (long long)sizeof(double);
  return 1;
}
