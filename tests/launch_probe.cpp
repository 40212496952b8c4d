// Records what lqer_linear_gemm_ld LAUNCHES, without a GPU: this program defines the few HIP entry points the GEMM's host code calls
// (a program's own symbols come first when the library it loads is bound), so every kernel launch lands in hipLaunchKernel below and
// is printed - kernel symbol, grid, workgroup, dynamic LDS bytes, and the two sizing arguments of the B_out pre-pass.  The device
// pointers handed in are never dereferenced by host code.  tests/test_launches_cpu.py builds it and holds its output to a record.
//   launch_probe LIBRARY CUS < cases      CUS: what the device query answers; one case per line: K N rank tuning  5 x (kind width block
//                                         exp_width exp_bias)  M dtype b_limbs
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/lqer_hip.h"

struct dim3 {
  uint32_t x, y, z;
};
static int g_cus = 256;

extern "C" {
int hipGetDevice(int* dev) { return *dev = 0; }
int hipDeviceGetAttribute(int* v, int, int) { return *v = g_cus, 0; }
int hipFuncSetAttribute(const void*, int, int) { return 0; }
int hipGetLastError(void) { return 0; }
static dim3 c_grid, c_block;  // the one pending <<<...>>> configuration
static size_t c_lds;
int __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, void*) { return c_grid = grid, c_block = block, c_lds = lds, 0; }
int __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, void** stream) {
  return *grid = c_grid, *block = c_block, *lds = c_lds, *stream = nullptr, 0;
}
int hipLaunchKernel(const void* f, dim3 grid, dim3 block, void** args, size_t lds, void*) {
  Dl_info info;
  const char* name = (dladdr(f, &info) && info.dli_sname) ? info.dli_sname : "?";
  printf(" %s %u,%u,%u %u %zu", name, grid.x, grid.y, grid.z, block.x, lds);
  if (strstr(name, "k_bout_amax")) printf(" [%d %d]", *(int*)args[1], *(int*)args[2]);
  return 0;
}
}

int main(int argc, char** argv) {
  void* lib = argc > 1 ? dlopen(argv[1], RTLD_NOW | RTLD_GLOBAL) : nullptr;
  if (argc > 2) sscanf(argv[2], "%d", &g_cus);
  if (!lib) return fprintf(stderr, "launch_probe: %s\n", dlerror()), 2;
  auto gemm = (decltype(&lqer_linear_gemm_ld))dlsym(lib, "lqer_linear_gemm_ld");
  auto limbs = (decltype(&lqer_desc_limbs))dlsym(lib, "lqer_desc_limbs");
  auto padded_r = (decltype(&lqer_padded_r))dlsym(lib, "lqer_padded_r");
  auto last_error = (decltype(&lqer_last_error))dlsym(lib, "lqer_last_error");
  void* const p = (void*)(uintptr_t)0x40000000;  // (aligned, never read)
  lqer_linear_desc_t d;
  long long M;
  int dtype, b_limbs;
  for (;;) {
    memset(&d, 0, sizeof(d));
    lqer_qfmt_t* f[5] = {&d.x_fmt, &d.w_fmt, &d.b_fmt, &d.a_out_fmt, &d.b_out_fmt};
    if (scanf("%d %d %d %d", &d.in_features, &d.out_features, &d.rank, &d.tuning) != 4) break;
    for (auto q : f)
      if (scanf("%d %d %d %d %d", &q->kind, &q->width, &q->block, &q->exp_width, &q->exp_bias) != 5) return 2;
    if (scanf("%lld %d %d", &M, &dtype, &b_limbs) != 3) return 2;
    int xl = 1, al = 1;
    limbs(&d, &xl, &al);
    const int rc = gemm(&d, p, M, p, d.rank > 0 ? p : nullptr, padded_r(d.rank) * al, d.rank > 0 ? p : nullptr, b_limbs, nullptr, p, dtype,
                        d.out_features, p, (size_t)1 << 40, nullptr);
    printf(" -> %d%s%s\n", rc, rc ? " " : "", rc ? last_error() : "");
  }
  return 0;
}
