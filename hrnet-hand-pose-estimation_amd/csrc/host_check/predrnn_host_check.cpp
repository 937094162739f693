// Stand-alone check of the HOST side of csrc/predrnn.hip under AddressSanitizer and UBSan, on the CPU: the partition of
// hrnet_sample_stats (csrc/predrnn_plan.h, through the query entry and directly) and every argument check of the four
// compute entries. No call here reaches a launch (each is refused first), so no GPU is needed and none is touched. Build
// and run, from the package directory:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I ../include -I csrc \
//         csrc/predrnn.hip csrc/host_check/predrnn_host_check.cpp -o predrnn_host_check && ./predrnn_host_check
//
// It supplies the two error-plumbing functions of api.hip itself, so that predrnn.hip links alone.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "hrnet_hip.h"
#include "predrnn_plan.h"

static char g_err[512];
static int g_launch_checks = 0;

void hr_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int hr_check_launch(const char*) {
  ++g_launch_checks;            // reached only after a launch: must stay 0 here
  return HR_E_LAUNCH;
}

static int failures = 0;

static void expect(bool ok, const char* what) {
  if (!ok) {
    ++failures;
    printf("FAILED: %s (last error: %s)\n", what, g_err);
  }
}

static void refused(int rc, const char* needle, const char* what) {
  expect(rc == HR_E_BADARG && strstr(g_err, needle) != nullptr, what);
  g_err[0] = 0;
}

int main() {
  // the partition over the cell's sizes and well beyond: every element belongs to exactly one part, no part is empty, the
  // maps' workgroups follow each other without a gap, two doubles of scratch per workgroup, and the entry agrees
  const long long sizes[] = {4, 8, 64, 8188, 8192, 8196, 8092, 44800, 1835008, 1048576, 786432, 262144, (1LL << 31) + 4};
  int asked = 0;
  for (int B : {1, 2, 3, 4, 17, 1000})
    for (long long n0 : sizes)
      for (long long n1 : sizes)
        for (long long n2 : {0LL, 4LL, 8192LL, 786432LL}) {
          const long long n[PRS_MAPS] = {n0, n1, n2};
          PrsPlan p;
          const int ok = prs_plan(B, n, &p);
          long long blocks = 0;
          bool fine = ok == 1 && p.maps == (n2 ? 3 : 2) && p.B == B;
          for (int m = 0; m < p.maps && fine; ++m) {
            const long long parts = p.parts[m];
            fine = p.first[m] == blocks && parts >= 1 && (parts - 1) * PRS_CHUNK < n[m] && n[m] <= parts * PRS_CHUNK;
            blocks += parts * B;
          }
          expect(fine && p.blocks == blocks && p.bytes == blocks * 16, "prs_plan: the parts cover every sample once");
          long long bytes = -1;
          expect(hrnet_sample_stats_scratch(B, n0, n1, n2, &bytes) == HR_OK && bytes == p.bytes, "sample_stats_scratch agrees");
          ++asked;
        }
  expect(asked > 1000, "prs_plan was hardly asked");
  long long bytes = -1;
  // one cell of the full-size model at B = 4: 7, 4 and 3 x 64 channels on 64 x 64 maps
  expect(hrnet_sample_stats_scratch(4, 1835008, 1048576, 786432, &bytes) == HR_OK && bytes == 4LL * (224 + 128 + 96) * 16,
         "the full-size cell: 224 + 128 + 96 parts per sample");
  expect(hrnet_sample_stats_scratch(1, 4, 0, 0, &bytes) == HR_OK && bytes == 16, "one map of four elements");
  refused(hrnet_sample_stats_scratch(1, 4, 0, 4, &bytes), "maps present first", "scratch: an absent map in front of a present one");
  refused(hrnet_sample_stats_scratch(1, 6, 0, 0, &bytes), "multiples of 4", "scratch: n = 6");
  refused(hrnet_sample_stats_scratch(0, 4, 0, 0, &bytes), "B = 0", "scratch: B = 0");
  refused(hrnet_sample_stats_scratch(1, 0, 0, 0, &bytes), "B = 1", "scratch: no map");
  refused(hrnet_sample_stats_scratch(1, -4, 0, 0, &bytes), "n = -4", "scratch: a negative size");
  refused(hrnet_sample_stats_scratch(0x7fffffff, 1LL << 40, 0, 0, &bytes), "2^31 - 1 parts", "scratch: too many workgroups");
  refused(hrnet_sample_stats_scratch(1, 4, 0, 0, nullptr), "null", "scratch: null bytes");

  alignas(16) float buf[1024] = {0};
  alignas(16) double scr[64] = {0};
  float* a = buf;
  float* b = buf + 256;
  float* c = buf + 512;
  float* d = buf + 768;
  const long long room = sizeof(scr);
  refused(hrnet_sample_stats(a, nullptr, nullptr, 6, 0, 0, 1, 1e-5, scr, room, d, nullptr), "multiples of 4", "stats n = 6");
  refused(hrnet_sample_stats(a, nullptr, nullptr, 4, 4, 0, 1, 1e-5, scr, room, d, nullptr), "go together", "stats size without a map");
  refused(hrnet_sample_stats(a, b, nullptr, 4, 0, 0, 1, 1e-5, scr, room, d, nullptr), "go together", "stats map without a size");
  refused(hrnet_sample_stats(a + 1, nullptr, nullptr, 4, 0, 0, 1, 1e-5, scr, room, d, nullptr), "16-byte", "stats alignment");
  refused(hrnet_sample_stats(a, nullptr, nullptr, 4, 0, 0, 1, 1e-5, nullptr, room, d, nullptr), "null", "stats null scratch");
  refused(hrnet_sample_stats(a, nullptr, nullptr, 4, 0, 0, 1, 1e-5, scr, room, nullptr, nullptr), "null", "stats null stats");
  refused(hrnet_sample_stats(a, nullptr, nullptr, 4, 0, 0, 1, 1e-5, scr, 15, d, nullptr), "15 bytes, 16 needed", "stats scratch one byte short");
  refused(hrnet_sample_stats(a, nullptr, nullptr, 4, 0, 0, 1, -1.0, scr, room, d, nullptr), "eps", "stats eps < 0");
  refused(hrnet_sample_stats(a, nullptr, nullptr, 1LL << 40, 0, 0, 0x7fffffff, 1e-5, scr, 0xffffffffLL, d, nullptr), "2^31 - 1 parts",
          "stats: more workgroups than a grid holds");

  // gates: B = 1, 2 x 2 maps, nh = 4; xc 112 floats in a, hc 64 and mc 48 in b, the affines and states in c, mem and o_pre in d
  float *xc = a, *hc = b, *mc = b + 64, *st = b + 128, *w = c, *ct = c + 128, *mt = c + 160, *mem = d, *op = d + 64;
#define GATES(xc_, ct_, ldc_, coff_, mt_, ldmt_, moff_, mem_, ldmem_, op_, B_, H_, W_, nh_) \
  hrnet_stlstm_gates(xc_, hc, mc, st, w, w, w, w, w, w, ct_, ldc_, coff_, mt_, ldmt_, moff_, mem_, ldmem_, op_, B_, H_, W_, nh_, nullptr)
  refused(GATES(nullptr, ct, 4, 0, mt, 4, 0, mem, 8, op, 1, 2, 2, 4), "null", "gates null xc");
  refused(GATES(xc, ct, 4, 0, mt, 4, 0, mem, 8, op, 1, 2, 2, 6), "nh = 6", "gates nh = 6");
  refused(GATES(xc, ct, 4, 0, mt, 4, 0, mem, 8, op, 0, 2, 2, 4), "B = 0", "gates B = 0");
  refused(GATES(xc, ct, 4, 0, mt, 4, 0, mem, 8, op, 1, 0x7fffffff, 0x7fffffff, 4), "too many", "gates: too many elements");
  refused(GATES(xc, ct, 6, 0, mt, 4, 0, mem, 8, op, 1, 2, 2, 4), "c_t channels", "gates ldc = 6");
  refused(GATES(xc, ct, 4, 4, mt, 4, 0, mem, 8, op, 1, 2, 2, 4), "c_t channels", "gates c_t slice outside its row");
  refused(GATES(xc, ct, 4, 0, mt, 4, -4, mem, 8, op, 1, 2, 2, 4), "m_t channels", "gates m_off < 0");
  refused(GATES(xc, ct, 4, 0, mt, 4, 0, mem, 4, op, 1, 2, 2, 4), "ldmem = 4", "gates: mem too narrow");
  refused(GATES(xc + 1, ct, 4, 0, mt, 4, 0, mem, 8, op, 1, 2, 2, 4), "16-byte", "gates alignment");
  refused(GATES(xc, mem, 8, 4, mt, 4, 0, mem, 8, op, 1, 2, 2, 4), "c_t overlaps mem", "gates: c_t is mem at the wrong offset");
  refused(GATES(xc, mem + 8, 8, 0, mt, 4, 0, mem, 8, op, 1, 2, 2, 4), "c_t overlaps mem", "gates: c_t is mem shifted by a pixel");
  refused(GATES(xc, mem, 8, 0, mem, 8, 0, mem, 8, op, 1, 2, 2, 4), "m_t overlaps mem", "gates: m_t is mem at the wrong offset");
  refused(GATES(xc, ct, 4, 0, mt, 4, 0, xc, 8, op, 1, 2, 2, 4), "an input overlaps", "gates: mem is xc");
  refused(GATES(xc, ct, 4, 0, mt, 4, 0, mem, 8, mem + 16, 1, 2, 2, 4), "o_pre overlaps", "gates: o_pre inside mem");
  refused(GATES(xc, ct, 4, 0, mt, 4, 0, mem, 8, ct, 1, 2, 2, 4), "o_pre overlaps", "gates: o_pre is c_t");

  //                       oc stats wo bo o_pre last h_new B  H  W  nh
  refused(hrnet_stlstm_out(a, st, w, w, b, c, nullptr, 1, 2, 2, 4, nullptr), "null", "out null h_new");
  refused(hrnet_stlstm_out(a, st, w, w, b, c, d, 1, 2, 2, 2, nullptr), "nh = 2", "out nh = 2");
  refused(hrnet_stlstm_out(a, st, w, w, b, c, d + 2, 1, 2, 2, 4, nullptr), "16-byte", "out alignment");
  refused(hrnet_stlstm_out(a, st, w, w, b, c, a, 1, 2, 2, 4, nullptr), "overlaps h_new", "out: h_new is oc");
  refused(hrnet_stlstm_out(a, st, w, w, b, c, c + 4, 1, 2, 2, 4, nullptr), "overlaps h_new", "out: h_new inside last");

  //                          x  y  N  H  W  C  ldx xo ldy yo
  refused(hrnet_maxpool2d_2x2(nullptr, d, 1, 2, 2, 4, 4, 0, 4, 0, nullptr), "null", "pool null x");
  refused(hrnet_maxpool2d_2x2(a, d, 1, 3, 2, 4, 4, 0, 4, 0, nullptr), "H = 3", "pool odd H");
  refused(hrnet_maxpool2d_2x2(a, d, 1, 2, 0, 4, 4, 0, 4, 0, nullptr), "W = 0", "pool W = 0");
  refused(hrnet_maxpool2d_2x2(a, d, 1, 2, 2, 3, 4, 0, 4, 0, nullptr), "multiples of 4", "pool C = 3");
  refused(hrnet_maxpool2d_2x2(a, d, 1, 2, 2, 4, 4, 4, 4, 0, nullptr), "outside ldx", "pool x slice");
  refused(hrnet_maxpool2d_2x2(a, d, 1, 2, 2, 4, 4, 0, 8, 8, nullptr), "outside ldy", "pool y slice");
  refused(hrnet_maxpool2d_2x2(a, d, 1, 2, 2, 4, 4, 0, 4, -4, nullptr), "outside ldy", "pool y_off < 0");
  refused(hrnet_maxpool2d_2x2(a, a + 4, 1, 2, 2, 4, 4, 0, 4, 0, nullptr), "overlap", "pool: y inside x");
  refused(hrnet_maxpool2d_2x2(a, d, 0x7fffffff, 0x7ffffffe, 2, 4, 4, 0, 4, 0, nullptr), "too many", "pool: too many elements");

  for (int i = 0; i < 1024; ++i) expect(buf[i] == 0.f, "a refused call wrote");
  for (int i = 0; i < 64; ++i) expect(scr[i] == 0.0, "a refused call wrote the scratch");
  expect(g_launch_checks == 0, "an argument check let a call through to a launch");
  printf(failures ? "predrnn host check: %d FAILED\n" : "predrnn host check: all answered as expected (%d)\n",
         failures ? failures : asked);
  return failures ? 1 : 0;
}
