// The host side of the one-launch decode forward (the kernels: decode1_kernel.h)
#include <atomic>

#include <cstdio>
#include <ctime>

#include "decode1_kernel.h"

namespace lqer {
namespace d1 {

static std::atomic<uint32_t> g_nonce{1};  // the call's granule tag: any value the granule area does not hold yet
static thread_local const char* g_why = "";  // why decode1_dispatch last answered LQER_E_UNSUPPORTED on this thread

}  // namespace d1

#ifdef LQER_D1_STAMPS
extern "C" int lqer_debug_set_d1_stamps(void* p) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(d1::g_d1_stamps), &p, sizeof(p)); }
#endif

const char* decode1_last_refusal() { return d1::g_why; }

size_t decode1_lds_bytes(int M, int64_t Kp, int cpw) {  // cpw: column blocks per consumer workgroup (one 8-KiB sum buffer each)
  const size_t xs = (size_t)M * ((Kp * 2 + 255) / 256 * 256), prod = d1::PSLAB_BYTES + d1::PRED_BYTES;  // (aliased: see the kernel)
  return (xs > prod ? xs : prod) + (size_t)cpw * d1::RED1_BYTES + d1::XAQ_BYTES + d1::FLAG_BYTES;
}

// ... of the NORM instantiations: the rows' statistics behind everything else (existing launches keep their size and their cpw)
static size_t decode1_lds_bytes_normed(int M, int64_t Kp, int cpw) { return decode1_lds_bytes(M, Kp, cpw) + d1::STAT_BYTES; }

size_t decode1_scratch_bytes(int64_t Kp, int rp) { return (size_t)((Kp + d1::SLAB_K - 1) / d1::SLAB_K) * d1::MAXM * rp * 8; }

// g: the shared part, filled like for the small-M kernel (M, Kp, aout, bout, tuning; xq / xaq / xa_part and the per-Linear fields
// unused) - mem[0 .. nmem-1]: the Linears of the launch (one, or a group that is handed the same tokens), a_t: the
// concatenation of their A^T images along the rank.  Returns LQER_E_UNSUPPORTED when the shape is outside.
// nz != nullptr: x is the raw hidden state h, and the kernel forms the norm of nz->norm (NORM_RMS, NORM_LAYER) itself - api.hip has
// checked the norm's operands (dtype, K, alignment); the NORM instantiations take standard images only.
// gz != nullptr: x is the gate projection's output, and the kernel forms h = act(x) * gz->up itself (one Linear, standard image; api.hip
// has checked act, the strides and the alignment).  No limit on K but the LDS image's.
int decode1_dispatch(GemmArgs g, int dtype, const void* x, int64_t ldx, int K, const QP& qx, const bf16_t* a_t, int bout,
                     const DecodeMember* mem, int nmem, void* scratch, size_t scratch_bytes, hipStream_t st, const DecodeNorm* nz,
                     const DecodeGate* gz) {
#ifdef LQER_HOST_TIMING
  timespec ht0; clock_gettime(CLOCK_MONOTONIC, &ht0);
#endif
  auto no = [](const char* why) {  // (nothing launched; the caller goes its own way and may quote the reason: decode1_last_refusal)
    d1::g_why = why;
    return LQER_E_UNSUPPORTED;
  };
  if (g.M < 1 || g.M > d1::MAXM || nmem < 1 || nmem > d1::MAXMEM || bout > 1) return no("1..8 tokens, 1..4 Linears, B_out pass-through or in blocks of 16");
  if (K % d1::K_STEP != 0) return no("in_features is not a multiple of 16");
  const int w_img = g.w_narrow >> 8;  // the compact image of a 2- / 3-bit weight: a single Linear's launch only
  if (w_img && (nmem != 1 || (w_img != 2 && w_img != 3))) return no("a compact weight image in a group, or of a width other than 2 or 3");
  if (nz && (w_img || (dtype != LQER_F16 && dtype != LQER_BF16) || K > arow::ROWS * arow::SLAB * 2))
    return no("the norm is formed for fp16 / bf16 tensors, standard weight images and in_features <= 8192");
  if (gz && (nz || nmem != 1 || w_img || (dtype != LQER_F16 && dtype != LQER_BF16)))
    return no("the gated MLP's h is formed for one Linear, fp16 / bf16 tensors and the standard weight image (a compact weight image: compute h)");
  d1::Args<d1::MAXMEM> a;
  int rp_all = 0, blocks = 0;
  for (int i = 0; i < nmem; ++i) {
    if (mem[i].rp <= 0 || mem[i].rp > 16 * d1::MAXNT || mem[i].rp % 16 || mem[i].Np % 16 || !mem[i].bt || mem[i].b_limbs < 1 ||
        mem[i].b_limbs > 3)
      return no("a Linear's padded rank (16..64), its B^T image or its limbs of B (1..3)");
    rp_all += mem[i].rp;
    blocks += mem[i].Np / 16;
  }
  if (rp_all > d1::MAX_RP_ALL) return no("the padded ranks sum to more than 128");
  if (scratch_bytes < decode1_scratch_bytes(g.Kp, rp_all) || ((uintptr_t)scratch & 15)) return no("the scratch is too small or not 16-byte aligned");
  a.np = (int)((g.Kp + d1::SLAB_K - 1) / d1::SLAB_K);
  // ONE round: at most what the chip holds at once (two workgroups per CU by registers, one when a workgroup's LDS - the x image
  // above all - takes more than half of the CU's); a consumer then walks `cpw` consecutive column blocks of its member.  The
  // smallest cpw whose own LDS footprint still leaves that many workgroups resident:
  constexpr int CUS = 256;
  size_t lds = 0;
  a.cpw = 0;
  for (int c = 1; c <= d1::MAXCPW; ++c) {
    lds = nz ? decode1_lds_bytes_normed(g.M, g.Kp, c) : decode1_lds_bytes(g.M, g.Kp, c);
    if (lds > 150 * 1024) break;
    const int slots = CUS * (2 * lds <= 160 * 1024 ? 2 : 1) - a.np;
    if (slots > 0 && (int64_t)slots * c >= blocks) {
      a.cpw = c;
      break;
    }
  }
  if (a.cpw == 0) return no("K too long for the LDS image, or more column blocks than one resident round of workgroups holds");
  int cbs = 0, roff = 0;
  for (int i = 0; i < nmem; ++i) {
    const int nblk = mem[i].Np / 16;
    a.mem[i] = d1::Member{mem[i].wp, mem[i].bt, mem[i].bias, mem[i].y, mem[i].ldy, mem[i].N, mem[i].Np, mem[i].rp, mem[i].b_limbs, roff, cbs, nblk};
    roff += mem[i].rp;
    cbs += (nblk + a.cpw - 1) / a.cpw;
  }
  for (int i = nmem; i < d1::MAXMEM; ++i) a.mem[i] = d1::Member{nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0, 0x7fffffff, 0};
  a.M = g.M, a.Kp = g.Kp, a.aout = g.aout, a.bout = g.bout;
  a.nmem = nmem, a.rp_all = rp_all;
  a.x = x, a.ldx = ldx, a.K = K, a.qx = qx, a.a_t = a_t;
  a.gran = (uint32_t*)scratch;
  // the call's tag: a counter spread over all 32 bits (odd multiplier: a bijection, so two calls never share a tag before
  // 2^32 calls) - small integers, zeros and the bit patterns of ordinary floats are what stale workspace bytes look like
  const uint32_t n = d1::g_nonce.fetch_add(1, std::memory_order_relaxed);
  a.nonce = n * 0x9E3779B1u ^ 0xA5C35A3Cu;
  a.spin = (g.tuning & LQER_TUNE_DECODE_NO_POLL) ? 0 : LQER_QD1_SPIN;  // (tests: every consumer computes the tiles itself)
  const unsigned grid = (unsigned)(a.np + cbs);
  d1::Args<1> a1;  // the single Linear's compact block
  a1.mem[0] = a.mem[0];
  a1.M = a.M, a1.Kp = a.Kp, a1.aout = a.aout, a1.bout = a.bout, a1.nmem = 1, a1.rp_all = a.rp_all, a1.x = a.x, a1.ldx = a.ldx, a1.K = a.K,
  a.w_exps = a1.w_exps = g.w_narrow & 0xff,
  a1.qx = a.qx, a1.a_t = a.a_t, a1.gran = a.gran, a1.nonce = a.nonce, a1.np = a.np, a1.spin = a.spin, a1.cpw = a.cpw;
#ifdef LQER_HOST_TIMING  // diagnostic build: host nanoseconds before / inside the launch call, printed at exit
  struct HostT {
    double pre = 0, launch = 0; long n = 0;
    ~HostT() { if (n) fprintf(stderr, "[decode1 host] calls %ld: dispatch before launch %.0f ns, launch call %.0f ns\n", n, pre / n, launch / n); }
  };
  static HostT host_t;
  timespec ht1; clock_gettime(CLOCK_MONOTONIC, &ht1);
#endif
  if (nz) {  // the NORM instantiations (decode1_normed.hip): the same blocks with the norm's operands behind them
    d1::ArgsN<d1::MAXMEM> an;
    d1::ArgsN<1> an1;
    (d1::Args<d1::MAXMEM>&)an = a, (d1::Args<1>&)an1 = a1;
    an.nz = an1.nz = d1::NormTail{nz->nw, nz->nb, nz->eps};
    return decode1_normed_launch(dtype, bout, nz->norm, grid, (int)lds, st, an, an1, nmem > 1);
  }
  if (gz) {  // the GATE instantiations (decode1_gated.hip): the single Linear's block with up behind it
    d1::ArgsG ag;
    (d1::Args<1>&)ag = a1;
    ag.gz = d1::GateTail{gz->up, gz->ld_up};
    return decode1_gated_launch(dtype, bout, gz->act, grid, (int)lds, st, ag);
  }
  const int rc = with_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value, LIMIT = 150 * 1024;
    const unsigned block = 64 * d1::NW;
    if (nmem > 1)
      return bout == 1 ? launch_k<d1::k_decode1<DT, 1, true>, LIMIT>("lqer_decode1", grid, block, (int)lds, st, a)
                       : launch_k<d1::k_decode1<DT, 0, true>, LIMIT>("lqer_decode1", grid, block, (int)lds, st, a);
    if (w_img == 2)
      return bout == 1 ? launch_k<d1::k_decode1_narrow<DT, 1, 2>, LIMIT>("lqer_decode1 (compact image)", grid, block, (int)lds, st, a1)
                       : launch_k<d1::k_decode1_narrow<DT, 0, 2>, LIMIT>("lqer_decode1 (compact image)", grid, block, (int)lds, st, a1);
    if (w_img == 3)
      return bout == 1 ? launch_k<d1::k_decode1_narrow<DT, 1, 3>, LIMIT>("lqer_decode1 (compact image)", grid, block, (int)lds, st, a1)
                       : launch_k<d1::k_decode1_narrow<DT, 0, 3>, LIMIT>("lqer_decode1 (compact image)", grid, block, (int)lds, st, a1);
    return bout == 1 ? launch_k<d1::k_decode1<DT, 1, false>, LIMIT>("lqer_decode1", grid, block, (int)lds, st, a1)
                     : launch_k<d1::k_decode1<DT, 0, false>, LIMIT>("lqer_decode1", grid, block, (int)lds, st, a1);
  });
#ifdef LQER_HOST_TIMING
  {
    timespec ht2; clock_gettime(CLOCK_MONOTONIC, &ht2);
    host_t.pre += (ht1.tv_sec - ht0.tv_sec) * 1e9 + (ht1.tv_nsec - ht0.tv_nsec);
    host_t.launch += (ht2.tv_sec - ht1.tv_sec) * 1e9 + (ht2.tv_nsec - ht1.tv_nsec);
    host_t.n++;
  }
#endif
  return rc;
}

}  // namespace lqer
