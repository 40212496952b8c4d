// Second half of the side path's split-K: the partial tiles of any side GEMM kernel -> A_out -> the bf16 image the GEMM's prologue reads.
#include "xa_common.h"

namespace lqer {
// Fixed-order sum over the chunks + A_out + bf16 store.  One lane per 4 consecutive rank entries; the G = L/4
// lanes of a block (G a power of two <= 64, lanes of one wave) share their max through xor-shuffles.
// MF (G = 1): a minifloat A_out - elementwise minifloat_value, |v| <= 1e-8 -> 0 as in every bf16 image.
template <int G, bool MF = false>
__global__ __launch_bounds__(256) void k_xa_reduce4(const float* __restrict__ part, XaPlan plan, int rp, QP q,
                                                    bf16_t* __restrict__ xaq, const float* __restrict__ rowscale = nullptr) {
  const int64_t total = (int64_t)plan.row_groups * XA_ROWS * rp / 4;  // float4 items (rp/4 per row, a multiple of G)
  const int64_t chunk_stride = (int64_t)plan.row_groups * XA_ROWS * rp;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (64-thread workgroups when the grid would not fill the chip)
  const bool live = idx < total;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    const float* src = part + idx * 4;
    // chunks summed in ascending order, 16 (then 8) loads in flight at a time: a launch-latency kernel, every round trip counts
    int c = 0;
    for (; c + 16 <= plan.nchunk; c += 16) {
      float4 v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = *(const float4*)(src + (c + u) * chunk_stride);
#pragma unroll
      for (int u = 0; u < 16; ++u) s.x += v[u].x, s.y += v[u].y, s.z += v[u].z, s.w += v[u].w;
    }
    for (; c + 8 <= plan.nchunk; c += 8) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = *(const float4*)(src + (c + u) * chunk_stride);
#pragma unroll
      for (int u = 0; u < 8; ++u) s.x += v[u].x, s.y += v[u].y, s.z += v[u].z, s.w += v[u].w;
    }
    for (; c < plan.nchunk; ++c) {
      const float4 v = *(const float4*)(src + c * chunk_stride);
      s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
    }
  }
  if (rowscale && live) {  // int8 activation image: the sums are of mantissas, the row's power-of-two scale comes last (exact)
    const float sc = rowscale[idx / (rp / 4)];
    s.x *= sc, s.y *= sc, s.z *= sc, s.w *= sc;
  }
  if constexpr (MF) {
    if (!live) return;
    const float v[4] = {s.x, s.y, s.z, s.w};
    uint32_t b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) b[i] = fabsf(v[i]) <= 1e-8f ? 0u : exact_bf16_bits(minifloat_value(v[i], q));
    *(uint2*)(xaq + idx * 4) = make_uint2(b[0] | (b[1] << 16), b[2] | (b[3] << 16));
    return;
  }
  float amax = fmaxf(fmaxf(fabsf(s.x), fabsf(s.y)), fmaxf(fabsf(s.z), fabsf(s.w)));
#pragma unroll
  for (int d = 1; d < G; d <<= 1) amax = fmaxf(amax, __shfl_xor(amax, d, 64));
  if (!live) return;
  const bool any = amax > 0.f;
  const int e = any ? block_exponent(amax, q) : 0;
  const float v[4] = {s.x, s.y, s.z, s.w};
  uint32_t w[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float m0v = any ? mxint_mantissa(v[2 * i], e, q) : 0.f;
    const float m1v = any ? mxint_mantissa(v[2 * i + 1], e, q) : 0.f;
    w[i] = exact_bf16_bits(ldexpf(m0v, e - q.mbits)) | (exact_bf16_bits(ldexpf(m1v, e - q.mbits)) << 16);
  }
  *(uint2*)(xaq + idx * 4) = make_uint2(w[0], w[1]);
}

// A_out_quantizer = passthrough (reference quantizers/passthrough.py:1; the *-int.toml templates leave A_out at the
// x quantizer's pass-through, linear.py:120-124): the fp32 sum is handed on as LA bf16 limbs laid side by side,
// xaq [rows][LA * rp], limb l of column n at l * rp + n (16 significand bits with two limbs - the reference keeps
// 11 (fp16 tensors) or 8 (bf16) here -, all 24 with three); B^T is repeated LA times along r to match.
template <int LA>
__global__ __launch_bounds__(256) void k_xa_reduce_limbs(const float* __restrict__ part, XaPlan plan, int rp,
                                                         bf16_t* __restrict__ xaq, const float* __restrict__ rowscale = nullptr) {
  const int64_t total = (int64_t)plan.row_groups * XA_ROWS * rp / 4;
  const int64_t chunk_stride = (int64_t)plan.row_groups * XA_ROWS * rp;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const float* src = part + idx * 4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  int c = 0;
  for (; c + 8 <= plan.nchunk; c += 8) {  // ascending, 8 loads in flight, as in k_xa_reduce4
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = *(const float4*)(src + (c + u) * chunk_stride);
#pragma unroll
    for (int u = 0; u < 8; ++u) s.x += v[u].x, s.y += v[u].y, s.z += v[u].z, s.w += v[u].w;
  }
  for (; c < plan.nchunk; ++c) {
    const float4 v = *(const float4*)(src + c * chunk_stride);
    s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
  }
  const int rq = rp / 4;
  const int64_t row = idx / rq;
  const int n0 = (int)(idx - row * rq) * 4;
  const float sc = rowscale ? rowscale[row] : 1.0f;
  float v[4] = {s.x * sc, s.y * sc, s.z * sc, s.w * sc};
#pragma unroll
  for (int l = 0; l < LA; ++l) {
    uint32_t w[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const bf16_t b0 = f32_to_bf16_rne(v[2 * i]), b1 = f32_to_bf16_rne(v[2 * i + 1]);
      v[2 * i] -= __uint_as_float((uint32_t)b0 << 16);
      v[2 * i + 1] -= __uint_as_float((uint32_t)b1 << 16);
      w[i] = (uint32_t)b0 | ((uint32_t)b1 << 16);
    }
    *(uint2*)(xaq + row * (LA * rp) + l * rp + n0) = make_uint2(w[0], w[1]);
  }
}

// Generic block length (not 4 * 2^g): one lane per block, serial.
__global__ __launch_bounds__(256) void k_xa_reduce_blk(const float* __restrict__ part, XaPlan plan, int rp, QP q,
                                                       bf16_t* __restrict__ xaq, const float* __restrict__ rowscale = nullptr) {
  const int L = (q.block <= 0 || q.block >= rp) ? rp : q.block;
  const int nb = rp / L;
  const int64_t total = (int64_t)plan.row_groups * XA_ROWS * nb;
  const int64_t chunk_stride = (int64_t)plan.row_groups * XA_ROWS * rp;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t row = idx / nb;
    const int b0 = (int)(idx - row * nb) * L;
    const float* src = part + row * rp + b0;
    bf16_t* dst = xaq + row * rp + b0;
    const float sc = rowscale ? rowscale[row] : 1.0f;
    float amax = 0.f;
    for (int k = 0; k < L; ++k) {
      float sum = src[k];
      for (int c = 1; c < plan.nchunk; ++c) sum += src[c * chunk_stride + k];
      amax = fmaxf(amax, fabsf(sum * sc));
    }
    const bool any = amax > 0.f;
    const int e = any ? block_exponent(amax, q) : 0;
    for (int k = 0; k < L; ++k) {
      float sum = src[k];
      for (int c = 1; c < plan.nchunk; ++c) sum += src[c * chunk_stride + k];
      sum *= sc;
      const float mv = any ? mxint_mantissa(sum, e, q) : 0.f;
      dst[k] = (bf16_t)exact_bf16_bits(ldexpf(mv, e - q.mbits));
    }
  }
}

// The one place that picks the reduce kernel (the dispatchers have refused what none takes)
void xa_reduce_launch(const float* part, const XaPlan& plan, int rp, const QP& q, int xa_limbs, bf16_t* xaq, const float* rowscale,
                      hipStream_t st) {
  const int64_t items = (int64_t)plan.row_groups * XA_ROWS * rp / 4;  // one lane per 4 consecutive rank entries
  const unsigned bs = items <= 128 * 256 ? 64 : 256;  // up to 32 Ki items (C2: 16 Ki): one wave per workgroup spreads them over all CUs
  const unsigned grid = (unsigned)((items + bs - 1) / bs), grid256 = (unsigned)((items + 255) / 256);
  const int L = xa_out_block(q, rp);
  if (q.kind == LQER_Q_MINIFLOAT) {  // elementwise
    k_xa_reduce4<1, true><<<grid, bs, 0, st>>>(part, plan, rp, q, xaq, rowscale);
  } else if (q.kind == LQER_Q_PASSTHROUGH) {  // the sum as 2 or 3 bf16 limbs
    if (xa_limbs == 2) k_xa_reduce_limbs<2><<<grid256, 256, 0, st>>>(part, plan, rp, xaq, rowscale);
    else k_xa_reduce_limbs<3><<<grid256, 256, 0, st>>>(part, plan, rp, xaq, rowscale);
  } else if (xa_reduce4_block(L)) {  // blocks of 4 * 2^g columns
    switch (L / 4) {
      case 1: k_xa_reduce4<1><<<grid, bs, 0, st>>>(part, plan, rp, q, xaq, rowscale); break;
      case 2: k_xa_reduce4<2><<<grid, bs, 0, st>>>(part, plan, rp, q, xaq, rowscale); break;
      case 4: k_xa_reduce4<4><<<grid, bs, 0, st>>>(part, plan, rp, q, xaq, rowscale); break;
      case 8: k_xa_reduce4<8><<<grid, bs, 0, st>>>(part, plan, rp, q, xaq, rowscale); break;
      case 16: k_xa_reduce4<16><<<grid, bs, 0, st>>>(part, plan, rp, q, xaq, rowscale); break;
      case 32: k_xa_reduce4<32><<<grid, bs, 0, st>>>(part, plan, rp, q, xaq, rowscale); break;
      default: k_xa_reduce4<64><<<grid, bs, 0, st>>>(part, plan, rp, q, xaq, rowscale); break;
    }
  } else {  // any other block length: one lane per block
    const int64_t total = (int64_t)plan.row_groups * XA_ROWS * (rp / L);
    k_xa_reduce_blk<<<(unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096), 256, 0, st>>>(part, plan, rp, q, xaq, rowscale);
  }
}

}  // namespace lqer
