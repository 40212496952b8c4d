// Stand-alone probe of the 4-bit weight expands of lqer_amd/csrc/common.h (built and run by tests/test_gpu_expand.py):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o expand_probe tests/expand_probe.hip && ./expand_probe
// expand_frag_lin rests on two facts about v_cvt_scalef32_pk_bf16_fp8 that no manual states: (a) e4m3 SUBNORMAL inputs (exponent
// field 0: the nibble's own magnitude bits) convert exactly, (b) the scale operand built as (exponent byte + 9) << 23 multiplies by
// exactly 2^(byte + 9 - 127).  Both are checked exhaustively: every value 0..255 of a packed byte (two nibbles: all 16 codes, -0
// included, in both nibble positions) in every byte position of the word, the other three bytes all zeros and all ones, times every
// exponent byte a weight image can hold and the linear form may see (1 .. LIN_EXP_BYTE_MAX; pack.hip clamps the byte to 1 .. 254).
// The table forms the kernels keep for the remaining images - expand_frag, and expand_frag_lut with the integer table, the tile
// kernel's fall-back - are checked over all of 1 .. 254, the bytes beyond LIN_EXP_BYTE_MAX included.
// Expected values are computed here on the host: element k of the fragment = +-magnitude * 2^(byte - 127) of nibble p (k = p / 2 for
// even p, 4 + p / 2 for odd p), as bf16 bits.  Prints one line per form; exit status 1 on any mismatch.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../lqer_amd/csrc/common.h"

using namespace lqer;

constexpr int WORDS = 256 * 4 * 2;  // byte value x byte position x background
constexpr uint32_t INT_LUT_LO = 0x44403800u, INT_LUT_HI = 0x4E4C4A48u;  // e4m3 bytes of 0..3 | 4..7

__host__ __device__ inline uint32_t probe_word(int w) {
  const uint32_t v = (uint32_t)(w & 255), pos = (uint32_t)((w >> 8) & 3), bg = (w >> 10) ? 0xffffffffu : 0u;
  return (bg & ~(0xffu << (8 * pos))) | (v << (8 * pos));
}

// FORM 0: expand_frag_lin, 1: expand_frag, 2: expand_frag_lut with the integer table.  out[(byte - 1) * WORDS + w] = the four dwords.
template <int FORM>
__global__ __launch_bounds__(256) void k_probe(int bytes, uint32_t lut_lo, uint32_t lut_hi, u32x4* __restrict__ out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= bytes * WORDS) return;
  const uint32_t eb = (uint32_t)(idx / WORDS) + 1u, word = probe_word(idx % WORDS);
  bf16x8 f;
  if constexpr (FORM == 0) f = expand_frag_lin(word, (eb + 9u) << 23);
  else if constexpr (FORM == 1) f = expand_frag(word, eb << 23);
  else f = expand_frag_lut(word, eb << 23, lut_lo, lut_hi);
  out[idx] = __builtin_bit_cast(u32x4, f);
}

static uint16_t expected_bits(uint32_t word, int k, int eb) {
  const int p = k < 4 ? 2 * k : 2 * (k - 4) + 1;
  const uint32_t nib = (word >> (4 * p)) & 0xfu;
  float v = ldexpf((float)(nib & 7u), eb - 127);  // exact: three significant bits, normal for every byte >= 1
  if (nib & 8u) v = -v;                           // (-0 keeps its sign)
  uint32_t b;
  memcpy(&b, &v, 4);
  return (uint16_t)(b >> 16);
}

#define HIP_OK(call)                                                          \
  do {                                                                        \
    const hipError_t e_ = (call);                                             \
    if (e_ != hipSuccess) {                                                   \
      fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));              \
      return 2;                                                               \
    }                                                                         \
  } while (0)

int main() {
  const char* names[3] = {"expand_frag_lin", "expand_frag", "expand_frag_lut(integer table)"};
  const int nbytes[3] = {LIN_EXP_BYTE_MAX, 254, 254};
  u32x4* d_out = nullptr;
  HIP_OK(hipMalloc(&d_out, (size_t)254 * WORDS * sizeof(u32x4)));
  std::vector<uint16_t> h((size_t)254 * WORDS * 8);
  long total_bad = 0;
  for (int form = 0; form < 3; ++form) {
    const int n = nbytes[form] * WORDS;
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (form == 0) k_probe<0><<<grid, 256>>>(nbytes[form], 0, 0, d_out);
    else if (form == 1) k_probe<1><<<grid, 256>>>(nbytes[form], 0, 0, d_out);
    else k_probe<2><<<grid, 256>>>(nbytes[form], INT_LUT_LO, INT_LUT_HI, d_out);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(h.data(), d_out, (size_t)n * sizeof(u32x4), hipMemcpyDeviceToHost));
    long bad = 0;
    for (int i = 0; i < n; ++i) {
      const int eb = i / WORDS + 1;
      const uint32_t word = probe_word(i % WORDS);
      for (int k = 0; k < 8; ++k) {
        const uint16_t want = expected_bits(word, k, eb), got = h[(size_t)i * 8 + k];
        if (want != got && bad++ < 8)
          printf("  %s: byte %d word %08x k %d: got %04x, expected %04x\n", names[form], eb, word, k, got, want);
      }
    }
    printf("%s: exponent bytes 1..%d x %d words x 8 elements: %ld mismatches\n", names[form], nbytes[form], WORDS, bad);
    total_bad += bad;
  }
  HIP_OK(hipFree(d_out));
  return total_bad ? 1 : 0;
}
