// Inference unit of the row16 attention forward (attn_fwd_row16.hip): the launch of the denoising step -- bf16, whole 16x16 planes,
// dim_head 128, one head, every row stride 128, no LSE / probe / stamps / ablations -- with the slab walk decided at compile time.
// Same algorithm as attn_fwd_row16_kernel<128, Big, 9, true, ...> and the same step bodies, slab images and epilogue, which both take
// from attn_row16_step.h: O is bit-identical (tests/test_attn_infer_unit_gpu.py compares the two routes; wmz_debug_attn_knobs(0, 1)
// keeps a launch on the run-time kernel).
//
// What the geometry fixes (H = W = 16, 16 waves, one chunk of 16 rows, two parity slabs of 8 rows per key plane):
//   * slab parity == LDS buffer: the walk is a loop over the workgroup's key planes whose body is the two slabs written out, every
//     LDS address `literal + lane base (+ step offset)`, every DMA destination `literal + 1 KB x wave`;
//   * a wave's slab rows lo .. hi of either parity, its third-piece predicate (wave + 32 < 36) and its per-lane DMA source offsets
//     are worked out once in the prologue;
//   * per plane the K and V plane pointers take one 64-bit add each; the wrap of the rotated plane order is the trip index at
//     which the pointers step back (t_wrap), known before the loop;
//   * the slab behind the last one is never requested: the issue is predicated (`more`), nothing else is;
//   * <3, 3> only: who owns a query row and who requests the next slab follow the work per slab (attn_slab_walk.h) -- wave w owns
//     row slab_wave_row(w), so that no SIMD carries more than 13 key rows of a slab, and the nine lightest waves of a slab request
//     the whole next one right behind the barrier, a class of pieces mod 9 each from ONE offset register; a wave with four key
//     rows requests nothing (profiles/attn_issue_plan/README.md);
//   * block -> (batch, query plane) and the rotated order's phase by the host's multipliers (div_m31), token indices in 32 bits:
//     wmz_attn_fwd_row16_infer_takes bounds the launch accordingly.
// Left at run time: B, S, eS, the query planes (qs0, Sq: the cone and the sampler pass trailing planes) and the pointers.
// The time window is the symmetric one: a launch with eSf != eS (a causal model) is not the unit's and runs the run-time row kernel.
// Measurements, the listing's instruction counts and what was tried: profiles/attn_infer_unit/README.md.
// bfloat16 only: no *_f16.hip unit includes this file.
#include "attn_row16_step.h"

#ifdef WMZ_OP16_F16
#error "attn_fwd_row16_infer.hip is a bfloat16 unit"
#endif
// Diagnostic build only (tools/build_variant.py <tag> attn_fwd_row16_infer.hip -DWMZ_ATTN_INFER_TS; never the product, whose listing
// carries none of this): workgroup 0 stamps the shader clock per wave at the slots tools/ts_attn.py reads -- per slab j < 14 its own
// pieces landed (3 + 4 j), through the barrier (4 + 4 j), requests issued (5 + 4 j), steps done (6 + 4 j) -- into a device array
// that wmz_debug_attn_infer_stamps copies out.
#ifdef WMZ_ATTN_INFER_TS
__device__ unsigned long long attn_infer_stamps[16 * 64];
#define WMZ_ITS(slot) do { if (blockIdx.x == 0 && lane == 0) attn_infer_stamps[wave * 64 + (slot)] = __builtin_readcyclecounter(); } while (0)
#define WMZ_ITS_REAL(slot) do { if (blockIdx.x == 0 && lane == 0) attn_infer_stamps[wave * 64 + (slot)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define WMZ_ITS_SLAB(k) do { if (its_j < 14) WMZ_ITS((k) + 4 * its_j); } while (0)
#define WMZ_ITS_NEXT() (void)++its_j
#else
#define WMZ_ITS(slot) do { } while (0)
#define WMZ_ITS_REAL(slot) do { } while (0)
#define WMZ_ITS_SLAB(k) do { } while (0)
#define WMZ_ITS_NEXT() do { } while (0)
#endif

namespace {

constexpr int DH = 128, NW = Big::NW, KCR = Big::KC, RS = Big::RS;   // dim_head, waves = query rows, rows per slab, row stride of a slab
using I = Img<DH, Big>;                                    // padded LDS slab images; 1 KB DMA pieces, a wave's are wave + 16 i
static_assert(I::PK == 36 && I::PV == 36, "pieces 0 and 1 exist for every wave, piece 2 for waves 0 .. 3");
constexpr int KS = DH / 32, MT = DH / 16;
constexpr unsigned LD_B = 128u * 2u;                       // bytes per token row of q, k, v, o
constexpr unsigned ROW_B = 16u * LD_B;                     // bytes per plane row of 16 keys
constexpr long PLANE_B = 256l * LD_B;                      // bytes per key plane

// n / d with the host's multiplier m = ceil(2^31 / d) (magic_m31), for n d <= 2^31: the multiplier's excess e = m d - 2^31 < d adds
// n e / (d 2^31) < 1 / d to n / d, too little to reach the next integer
__device__ __forceinline__ unsigned div_m31(unsigned n, unsigned m) { return __umulhi(n << 1, m); }
unsigned magic_m31(unsigned d) { return (unsigned)(((1ull << 31) + d - 1) / d); }

// The issue plan of attn_slab_walk.h by wave, as literals: a nibble per wave with its class of pieces (0 where it never issues), and
// the waves that issue during the slab of parity `par`
constexpr unsigned long issue_classes() {
  unsigned long t = 0;
  for (int w = 0; w < NW; ++w) {
    const int c = slab_issue_class(slab_wave_row(w));
    t |= (unsigned long)(c < 0 ? 0 : c) << (4 * w);
  }
  return t;
}
constexpr unsigned issuers(int par) {
  unsigned m = 0;
  for (int w = 0; w < NW; ++w) m |= (unsigned)slab_issues(slab_wave_row(w), par) << w;
  return m;
}

template <int EH, int EW>
__global__ __launch_bounds__(NW * 64, 4) void attn_fwd_row16_infer_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K,
                                                                        const bf16_t* __restrict__ V, bf16_t* __restrict__ O,
                                                                        int S, int eS, int qs0, int Sq, float scale,
                                                                        unsigned m_sq, unsigned m_win) {
  static_assert(EH == 3 || EH == 1, "the steps of a slab are written out for these row extents");
  __shared__ __attribute__((aligned(1024))) char smem[2 * I::BUF];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, li = lane & 15;
#ifdef WMZ_ATTN_INFER_TS
  int its_j = 0;                                        // slab index of the stamps
#endif
  WMZ_ITS(0); WMZ_ITS_REAL(60);

  // xcd_remap (wmz_common.h) without its branch: XCD x takes the logical ids from x q + min(x, r) on (q = grid / 8, r = grid % 8)
  const unsigned xcd = blockIdx.x & 7u;
  const unsigned lid = xcd * (gridDim.x >> 3) + min(xcd, gridDim.x & 7u) + (blockIdx.x >> 3);
  const int b = (int)div_m31(lid, m_sq);                // lid / Sq
  const int sq = (int)(lid - (unsigned)b * (unsigned)Sq);
  const int s = qs0 + sq;
  constexpr bool PLAN = EH == 3;                        // <3, 3>: row map and issue plan of attn_slab_walk.h
  int hq = wave;                                        // this wave's query row
  if constexpr (PLAN) hq = slab_wave_row(wave);         // ... spread so that no SIMD carries more than 13 key rows of a slab
  const unsigned tok_q = (unsigned)(b * S + s) * 256u + (unsigned)(hq * 16);     // first token of this wave's query row, of its output row
  const unsigned tok_o = lid * 256u + (unsigned)(hq * 16);                       // (32-bit token indices: the hand-over bounds them)
  const float c2 = scale * 1.4426950408889634f;

  // bm[r] = column-window bias of this lane's key column (w = 4g + r) against its query (w = li), minus the running max
  float bm[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int d = 4 * g + r - li;
    bm[r] = (d <= EW && -d <= EW) ? 0.f : -INFINITY;
  }

  Frag8<bf16_t> qf[KS];
  f32x4 o[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) o[mt] = (f32x4)(0.f);
  float m_run = 0.f, l_run = 0.f;                        // m_run: log2 units of the scaled logits; set by the first step
  // the deferred-maximum rule's threshold: the reference moves when some logit exceeds it by more than 2^DEFER -- and at the wave's
  // very first step, whatever the logits: until then the threshold is -inf (wave-uniform; a step always holds a finite logit)
  float thr = -INFINITY;

  const int kbase = li * I::KROW + g * 16;
  const int vbase = I::KIMG + (4 * g + (li >> 2)) * I::VROW + (li & 3) * 8;
  // slab rows this wave needs, per parity (slab row r of parity p is plane row p + 2 r)
  const int my_lo = max(hq - EH, 0), my_hi = min(hq + EH, 15);
  const int lo0 = max(0, (my_lo + RS - 1) >> 1), hi0 = min(KCR - 1, my_hi >> 1);
  const int lo1 = max(0, (my_lo - 1 + RS - 1) >> 1), hi1 = min(KCR - 1, (my_hi - 1) >> 1);
  const bool has2 = wave + 2 * NW < I::PK;              // this wave's third piece of either image exists

  // per-lane source offsets of the wave's DMA pieces (whole planes: they never change)
  // (issue plan: only the first slab is requested this way; from then on a wave owns one class of pieces mod 9, both images from pvo)
  unsigned kvo[3], vvo[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) kvo[i] = piece_voff<DH, I::KROW, RS>(wave + NW * i, lane, LD_B, 16 - RS);
#pragma unroll
  for (int i = 0; i < 3; ++i) vvo[i] = piece_voff<DH, I::VROW, RS>(wave + NW * i, lane, LD_B, 16 - RS);

  // key planes in the rotated order of attn_slab_walk.h (slab_first_plane): from p_first up to the window's last plane, then from
  // its first one up to p_first - 1
  const int sk_lo = max(0, s - eS), sk_hi = min(S - 1, s + eS);
  const int nplanes = sk_hi - sk_lo + 1;
  const int nwin = 2 * eS + 1;
  int p_first = s - eS;
  {                                                     // first plane of the window with S-1-p = 0 (mod nwin); S-1-p_first >= eS >= 0
    const unsigned d = (unsigned)(S - 1 - p_first);
    p_first += (int)(d - div_m31(d, m_win) * (unsigned)nwin);
  }
  if (p_first > sk_hi || p_first < sk_lo) p_first = sk_lo;
  const unsigned long pl_b = (unsigned long)(unsigned)(b * S + p_first) * (unsigned long)PLANE_B;
  const char* kpl = (const char*)K + pl_b;                                       // plane of the slab being requested
  const char* vpl = (const char*)V + pl_b;
  const int t_wrap = sk_hi - p_first;                                            // behind this trip the pointers step back to sk_lo
  const long back = -(long)(nplanes - 1) * PLANE_B;

  int wdst = wave * 1024;                                // LDS offset of the wave's piece 0 of the K image of buffer 0
  // issue plan: the wave's class of pieces (0 where it never issues), whether it issues during the slab of parity 0 / 1, its per-lane
  // source offset (the K and the V image share row pitch and width, hence the offsets) and the LDS offset of its piece 0
  static_assert(I::KROW == I::VROW, "one offset register serves both images");
  int cdst = 0;
  unsigned pvo = 0;
  bool iss0 = false, iss1 = false;
  if constexpr (PLAN) {
    constexpr unsigned long CLS = issue_classes();
    constexpr unsigned ISS0 = issuers(0), ISS1 = issuers(1);
    const int cls = (int)(CLS >> (4 * wave)) & 15;
    iss0 = (ISS0 >> wave) & 1u; iss1 = (ISS1 >> wave) & 1u;
    pvo = piece_voff<DH, I::KROW, RS>(cls, lane, LD_B, 16 - RS);
    cdst = cls * 1024;
  }
  auto issue_c = [&](auto par, auto jc, int img, const char* p) {
    constexpr int PAR = decltype(par)::value, j = decltype(jc)::value;
    __builtin_amdgcn_global_load_lds((gptr_t)((p + PAR * ROW_B) + (pvo + j * SLAB_CLASS_STEP)), (lptr_t)(smem + cdst + PAR * I::BUF + img + j * 9 * 1024), 16, 0, 0);
  };
  // request this wave's pieces of a slab: K image of parity PAR from kp, V image from vp, into LDS buffer PAR
  auto issue_k = [&](auto par, auto ic, const char* kp) {
    constexpr int PAR = decltype(par)::value, i = decltype(ic)::value;
    __builtin_amdgcn_global_load_lds((gptr_t)((kp + PAR * ROW_B) + kvo[i]), (lptr_t)(smem + wdst + PAR * I::BUF + i * NW * 1024), 16, 0, 0);
  };
  auto issue_v = [&](auto par, auto ic, const char* vp) {
    constexpr int PAR = decltype(par)::value, i = decltype(ic)::value;
    __builtin_amdgcn_global_load_lds((gptr_t)((vp + PAR * ROW_B) + vvo[i]), (lptr_t)(smem + wdst + PAR * I::BUF + I::KIMG + i * NW * 1024), 16, 0, 0);
  };
  using C0 = std::integral_constant<int, 0>;
  using C1 = std::integral_constant<int, 1>;
  using C2 = std::integral_constant<int, 2>;

  // ---- rare branch of the online softmax: move the running max by the cross-lane maximum `gm` of the step
  auto rescale = [&](float mx, auto& t) {
    constexpr int nt = (int)(sizeof(t) / sizeof(float));
    float gm = wave_groups_max(mx);
    // behind the first step the reference only moves up: gm = max(gm, 0).  The first step sets it, to whatever sign: its floor is
    // thr - DEFER = -inf, and o and l, still zero, are multiplied by an alpha held at 1 or below (min: the identity once gm >= 0)
    gm = fmaxf(gm, thr - DEFER);
    const float alpha = __builtin_amdgcn_exp2f(fminf(-gm, 0.f));
    l_run *= alpha;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) o[mt] *= alpha;
    thr = DEFER;
    m_run += gm;
#pragma unroll
    for (int r = 0; r < 4; ++r) bm[r] = (bm[r] == -INFINITY) ? -INFINITY : -m_run;
#pragma unroll
    for (int r = 0; r < nt; ++r) t[r] -= gm;
  };

  auto hot = [&](float mx) { return __any(mx > thr); };
  // ---- two key rows (slab rows t0, t0 + 1 of buffer PAR): 32 keys.  vnow (<1, 1>): this is the wave's step of the slab and carries the
  // requests for V pieces 0 and 1 of the next slab (schedule 1 of attn_fwd_row16.hip: behind the QK^T MFMAs and behind the softmax)
  auto step2 = [&](auto par, int t0, bool vnow, const char* vp) {
    constexpr int PAR = decltype(par)::value;
    using NX = std::integral_constant<int, 1 - PAR>;
    const char* Sb = smem + PAR * I::BUF;
    const int ko = kbase + t0 * 16 * I::KROW;
    const unsigned va0 = lds_addr(Sb + vbase + t0 * 16 * I::VROW), va1 = va0 + 16 * I::VROW;
    attn_step32<I::KROW>(Sb, ko, va0, va1, qf, o, bm, c2, l_run, hot, rescale, StepNop{}, StepNop{}, [&](auto pc) {
      constexpr int pt = decltype(pc)::value;
      if constexpr (pt <= 2) { if (vnow) issue_v(NX{}, std::integral_constant<int, pt - 1>{}, vp); }
    });
  };
  // ---- odd last key row of the slab: a 16-key step
  auto step1 = [&](auto par, int t0) {
    constexpr int PAR = decltype(par)::value;
    const char* Sb = smem + PAR * I::BUF;
    const int ko = kbase + t0 * 16 * I::KROW;
    const unsigned va0 = lds_addr(Sb + vbase + t0 * 16 * I::VROW);
    attn_step16(Sb, ko, va0, qf, o, bm, c2, l_run, hot, rescale, StepNop{}, StepNop{});
  };
  // ---- one slab: buffer PAR holds parity PAR of the current plane; `more`: the next slab (parity 1 - PAR, of the plane kp / vp
  // point at) is requested into the other buffer -- <1, 1>: K behind the barrier, V inside the step, the rest behind it; <3, 3>,
  // the issue plan: K and V behind the barrier, by the waves that have fewer than four rows in this slab
  auto slab = [&](auto par, bool more, const char* kp, const char* vp) {
    constexpr int PAR = decltype(par)::value;
    using NX = std::integral_constant<int, 1 - PAR>;
    // (the offsets are taken afresh in every slab: hoisted out of the plane loop, the compiler keeps twelve more scalars for the
    //  destinations and widens the source offsets to register pairs, which costs the DMA its scalar-base + 32-bit-offset form)
    if constexpr (PLAN) asm volatile("" : "+s"(cdst), "+v"(pvo));
    else asm volatile("" : "+s"(wdst), "+v"(kvo[0]), "+v"(kvo[1]), "+v"(kvo[2]), "+v"(vvo[0]), "+v"(vvo[1]), "+v"(vvo[2]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's pieces of the slab landed
    WMZ_ITS_SLAB(3);
    __builtin_amdgcn_s_barrier();                        // ... everyone's did, and the slab before is retired: refill its buffer
    WMZ_ITS_SLAB(4);
    if constexpr (PLAN) {
      // a wave with fewer than four rows in this slab requests its class of the next one, K then V, before its own step; a wave
      // with four rows requests nothing and starts computing at once
      if (more && (PAR ? iss1 : iss0)) {
        static_for<4>([&](auto j) { issue_c(NX{}, j, 0, kp); });
        static_for<4>([&](auto j) { issue_c(NX{}, j, I::KIMG, vp); });
      }
    } else if (more) {
      issue_k(NX{}, C0{}, kp); issue_k(NX{}, C1{}, kp);
      if (has2) issue_k(NX{}, C2{}, kp);
    }
    WMZ_ITS_SLAB(5);
    // the wave's rows lo .. hi of this slab: two a step from lo, an odd last row as the 16-key step.  Of the window's 2 EH + 1 rows no
    // fewer than EH + 1 lie in the plane, so a parity has (EH + 1) / 2 .. EH + 1 of them.
    const int lo = PAR ? lo1 : lo0, hi = PAR ? hi1 : hi0;
    if constexpr (EH == 3) {
      // 2 .. 4 rows: one or two two-row steps, none of which carries a request.  (One copy of either step per slab: a peeled first
      // step would double the listing for the sake of two uniform branches.)
      int t0 = lo;
#pragma clang loop unroll(disable)
      do { step2(par, t0, false, vp); t0 += 2; } while (t0 + 1 <= hi);
      if (t0 <= hi) step1(par, t0);
    } else {
      // 1 or 2 rows: one step; what the odd one does not carry goes out behind it
      int t0 = lo;
      if (t0 < hi) { step2(par, t0, more, vp); t0 += 2; }
      if (t0 <= hi) {
        step1(par, t0);
        if (more) { issue_v(NX{}, C0{}, vp); issue_v(NX{}, C1{}, vp); }
      }
      // whatever of the next slab has not been requested yet
      if (more && has2) issue_v(NX{}, C2{}, vp);
    }
    WMZ_ITS_SLAB(6); WMZ_ITS_NEXT();
  };

  // the first slab is requested up front
  issue_k(C0{}, C0{}, kpl); issue_k(C0{}, C1{}, kpl);
  issue_v(C0{}, C0{}, vpl); issue_v(C0{}, C1{}, vpl);
  if (has2) { issue_k(C0{}, C2{}, kpl); issue_v(C0{}, C2{}, vpl); }
  WMZ_ITS(2);
  {
    // Q right behind the first slab's requests
    const bf16_t* qrow = Q + (unsigned long)tok_q * 128ul + (unsigned)(li * 128);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) frag_load(qf[ks], qrow + ks * 32 + g * 8);
  }
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks].v));   // Q is waited for HERE, once (the compiler's wait is vmcnt(0): inside
                                                                       // the loop it would drain the slabs in flight at every iteration)
  int t = 0;
  do {                                                   // (nplanes >= 1: the query plane itself)
    slab(C0{}, true, kpl, vpl);                          // parity 0; requests parity 1 of the same plane
    const long mv = t == t_wrap ? back : PLANE_B;
    kpl += mv; vpl += mv;                                // the next plane of the rotated order
    slab(C1{}, t + 1 < nplanes, kpl, vpl);               // parity 1; requests parity 0 of the next plane, if there is one
  } while (++t < nplanes);
  WMZ_ITS(63);

  {
    float l = wave_groups_sum(l_run);
    const float inv = 1.f / l;
    bf16_t* orow = O + (unsigned long)tok_o * 128ul + (unsigned)(li * 128);
    WMZ_ATTN_STORE_EPI16(o, inv, orow, g);
  }
  WMZ_ITS(62); WMZ_ITS_REAL(61);
}

template <int EH, int EW>
int launch_infer(const void* q, const void* k, const void* v, void* out, const AttnGeom& G, hipStream_t st) {
  const long nwg = (long)G.B * G.Sq;
  hipLaunchKernelGGL((attn_fwd_row16_infer_kernel<EH, EW>), dim3((unsigned)nwg), dim3(NW * 64), 0, st, (const bf16_t*)q,
                     (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)out, G.S, G.eS, G.qs0, G.Sq, G.scale,
                     magic_m31((unsigned)G.Sq), magic_m31(2u * (unsigned)G.eS + 1u));
  WMZ_LAUNCH_CHECK("wmz_local3d_attn_fwd(row16 infer)");
  return WMZ_OK;
}

}  // namespace

// Whether a launch is the unit's: what the kernels above fix at compile time (attn_fwd_impl adds what it alone knows: the dtype,
// no LSE, no probe, no stamp buffer).
bool wmz_attn_fwd_row16_infer_takes(const AttnGeom& G) {
  return G.eSf == G.eS && G.W == 16 && G.H == 16 && G.dh == 128 && G.heads == 1 && G.ldq == 128 && G.ldk == 128 && G.ldv == 128 && G.ldo == 128 &&
         ((G.eH == 3 && G.eW == 3) || (G.eH == 1 && G.eW == 1)) && G.dbg == 0 && G.variant == 0 && G.w8 == 0 &&
         (long)G.B * G.S * 256 <= (1l << 31) && (long)G.B * G.Sq * G.Sq <= (1l << 31) && ((long)G.S + G.eS) * (2l * G.eS + 1) <= (1l << 31);       // 32-bit tokens, div_m31's range
}

#ifdef WMZ_ATTN_INFER_TS
extern "C" int wmz_debug_attn_infer_stamps(unsigned long long* out, int n) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(attn_infer_stamps), (size_t)n * sizeof(unsigned long long));
}
#endif

int wmz_attn_fwd_row16_infer_dispatch(const void* q, const void* k, const void* v, void* out, const AttnGeom& G, hipStream_t st) {
  if (G.eH == 3) return launch_infer<3, 3>(q, k, v, out, G, st);
  return launch_infer<1, 1>(q, k, v, out, G, st);
}
