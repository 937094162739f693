// The launch plan of hrnet_conv2d_kxk_wgrad (csrc/conv_kxk_train.hip): plain host arithmetic in a header of its own so
// that csrc/host_check/conv_kxk_train_host_check.cpp runs it under the sanitizers without a device.
//
// A workgroup owns one (16 output channels) x (16 input channels) block of dW - with Cin == 4 (the image layers) one
// (16 output channels) x (all 4 input channels) block - for ALL taps, and a contiguous range of 8 x 16 pixel tiles:
// split k walks tiles [k * per, min((k + 1) * per, tiles)), tiles numbered n-major, then tile row, then tile column.
// The split count aims at KXW_TARGET_WG workgroups (four per CU of a 256-CU device) and depends on the shape alone:
//   want = ceil(KXW_TARGET_WG / blocks); nsplit0 = min(tiles, want, KXW_MAX_SPLIT); per = ceil(tiles / nsplit0);
//   nsplit = ceil(tiles / per)          (no split is empty)
// Scratch: nsplit x (blocks x units x 256 + 16 cot) floats, units = ks * ks (or ks * ceil(ks / 4) four-tap groups with
// Cin == 4), the trailing 16 cot floats of a split being its bias-gradient partial.
#pragma once

constexpr int KXW_TH = 8, KXW_TW = 16, KXW_TARGET_WG = 1024, KXW_MAX_SPLIT = 128, KXW_MAXKS = 11;

struct KxwPlan {
  int cin4, cot, cit, units, tiles_h, tiles_w, nsplit;
  long long blocks, tiles, per, split_floats, bytes;
};

// 0 if the shape cannot be planned (counts beyond what a grid or a 64-bit size holds); arguments are assumed >= 1
inline int kxw_plan(int N, int H, int W, int Cin, int Cout, int ks, KxwPlan* p) {
  p->tiles_h = (int)(((long long)H + KXW_TH - 1) / KXW_TH);
  p->tiles_w = (int)(((long long)W + KXW_TW - 1) / KXW_TW);
  const long long t1 = (long long)N * p->tiles_h;
  if (t1 > 0x7fffffffLL) return 0;
  p->tiles = t1 * p->tiles_w;
  if (p->tiles > 0x7fffffffLL) return 0;
  p->cin4 = Cin == 4;
  p->cot = (int)(((long long)Cout + 15) / 16);
  p->cit = p->cin4 ? 1 : (int)(((long long)Cin + 15) / 16);
  p->units = p->cin4 ? ks * ((ks + 3) / 4) : ks * ks;
  p->blocks = (long long)p->cot * p->cit;
  if (p->blocks > 0x7fffffffLL) return 0;
  long long want = (KXW_TARGET_WG + p->blocks - 1) / p->blocks;
  if (want < 1) want = 1;
  long long n0 = p->tiles < want ? p->tiles : want;
  if (n0 > KXW_MAX_SPLIT) n0 = KXW_MAX_SPLIT;
  p->per = (p->tiles + n0 - 1) / n0;
  p->nsplit = (int)((p->tiles + p->per - 1) / p->per);
  p->split_floats = p->blocks * p->units * 256 + (long long)p->cot * 16;   // < 2^31 * 121 * 256 + 2^31: fits
  p->bytes = p->split_floats * p->nsplit * 4;                               // < 2^46 * 2^7 * 4
  return 1;
}
