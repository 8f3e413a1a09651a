// The rules of csrc/sf_launch_plan.h, one printed line per case: tests/test_launch_plan_cpu.py builds this with the host compiler (C++17, address and
// undefined-behaviour sanitizers), runs it and compares every line with the formulas the launchers had written out before the header existed.
#include "sf_launch_plan.h"

#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>

static const char* const VAR = "SF_LAUNCH_PLAN_TEST_KNOB";

static int knob_once() {
  static const int v = sf_env_int(VAR, 5);        // the form of every call site
  return v;
}

static void tile_case(long long M, long long N, int BM, int BN) {
  uint32_t tiles_n = 0, total = 0;
  if (sf_tile_counts(M, N, BM, BN, &tiles_n, &total)) printf("tile_counts %lld %lld %d %d ok %u %u\n", M, N, BM, BN, tiles_n, total);
  else printf("tile_counts %lld %lld %d %d refused\n", M, N, BM, BN);
}

int main() {
  const int n_cus[] = {1, 7, 8, 9, 255, 256, 304};
  const long long items[] = {1, 7, 8, 9, 255, 256, 257, 2147483647LL};
  for (int n_cu : n_cus) {
    for (long long it : items) printf("xcd_grid %d %lld %lld\n", n_cu, it, (long long)sf_xcd_grid(n_cu, it));
    printf("xcd_grid %d uncapped %lld\n", n_cu, (long long)sf_xcd_grid(n_cu));
    for (long long t : {1LL, (long long)n_cu - 1, (long long)n_cu, (long long)n_cu + 1}) printf("cu_grid %d %lld %lld\n", n_cu, t, (long long)sf_cu_grid(n_cu, t));
  }

  tile_case(255, 63, 256, 256);
  tile_case(256, 256, 256, 256);
  tile_case(257, 257, 256, 256);
  tile_case(14492, 1280, 256, 256);
  tile_case(1, 1, 128, 128);
  tile_case(2147483647LL * 256 - 255, 256, 256, 256);      // (2^31 - 1) x 1 tiles: the largest count that is served
  tile_case(65536LL * 256, 32768LL * 256 - 255, 256, 256); // 65536 x 32768 = 2^31 tiles: refused

  for (long long K : {64, 128, 256, 768, 1024, 1088, 3072}) printf("l2_nchunk bf16 %lld %u\n", K, sf_l2_nchunk(K, 512, 1024));
  for (long long K : {128, 768, 2048, 2176}) printf("l2_nchunk mxfp8 %lld %u\n", K, sf_l2_nchunk(K, 256, 2048));

  unsetenv(VAR);
  printf("env_int unset %d\n", sf_env_int(VAR, 7));
  for (const char* s : {"0", "12", "-3"}) {
    setenv(VAR, s, 1);
    printf("env_int %s %d\n", s, sf_env_int(VAR, 7));
  }
  setenv(VAR, "12", 1);
  const int first = knob_once();
  setenv(VAR, "34", 1);
  printf("env_static %d %d %d\n", first, knob_once(), sf_env_int(VAR, 7));
  return 0;
}
