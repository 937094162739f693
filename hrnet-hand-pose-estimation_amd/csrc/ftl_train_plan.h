// The launch plan of hrnet_conv2d_3x3g_wgrad (csrc/ftl_train.hip): plain host arithmetic in a header of its own so that
// csrc/host_check/ftl_train_host_check.cpp runs it under the sanitizers without a device.
//
// The plan of csrc/conv_kxk_split.h fits as it stands once its pixel tiles are those of the OUTPUT map (the dy of the
// weight gradient, Ho x Wo): a workgroup owns one (16 output channels) x (16 input channels) block of dW for all nine
// taps and a contiguous range of 8 x 16 output-pixel tiles, split k walks tiles [k * per, min((k + 1) * per, tiles)),
// n-major, then tile row, then tile column. The four-channel arrangement of the image layers is not built here: a
// 4-channel input is planned as one 16-channel block like any other. The bias slot at the end of a split's scratch
// (16 cot floats) belongs to the plan and stays unwritten: this entry has no bias gradient.
//
// g3w_size_range: the output sizes hrnet_conv2d_3x3g takes along an axis of n inputs at z = 1: between the size with no
// padding behind the map and that with two rows of it.
#pragma once

#include "conv_kxk_split.h"

inline void g3w_size_range(int n, int stride, int pad_lo, long long* lo, long long* hi) {
  const long long m = (long long)n + pad_lo;
  *lo = m - 3 < 0 ? 1 : (m - 3) / stride + 1;
  *hi = (m - 1) / stride + 1;
}

// 0 if the shape cannot be planned; arguments are assumed >= 1
inline int g3w_plan(int N, int Ho, int Wo, int Cin, int Cout, KxwPlan* p) {
  return kxw_plan(N, Ho, Wo, Cin == 4 ? 8 : Cin, Cout, 3, p);
}
