// Error plumbing and version of libwmz_hip.so, plus the token/position embedding kernel.
#include "wmz_common.h"
#include "fused_row_maps.h"
#include <string.h>

static thread_local char g_err[512] = "";

void wmz_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" int wmz_version(void) { return WMZ_VERSION; }
extern "C" const char* wmz_last_error(void) { return g_err; }

// ---- the half guard's binding (wmz_common.h HalfGuard): every guarded unit registers the setter of its own __constant__ copy of
// the word's address from a static constructor, so the table lives behind a function (initialised on first use, whatever the
// order the units' constructors run in)
typedef int (*wmz_hg_setter)(unsigned*);
namespace {
struct HgUnits { wmz_hg_setter set[32]; int n; };       // (n counts every registration: one past the table is an error at bind)
HgUnits& hg_units() { static HgUnits u = {{nullptr}, 0}; return u; }
}
void wmz_half_guard_register_unit(wmz_hg_setter set) {
  HgUnits& u = hg_units();
  if (u.n < 32) u.set[u.n] = set;
  ++u.n;
}
extern "C" int wmz_half_guard_bind(void* word) {
  WMZ_REQUIRE(((uintptr_t)word & 3) == 0, "wmz_half_guard_bind: the word must be 4-byte aligned");
  const HgUnits& u = hg_units();
  WMZ_REQUIRE(u.n <= 32, "wmz_half_guard_bind: %d guarded units registered, the table holds 32: a unit would stay unguarded", u.n);
  for (int i = 0; i < u.n; ++i)
    if (u.set[i]((unsigned*)word) != 0) {
      wmz_set_error("wmz_half_guard_bind: symbol copy failed: %s", hipGetErrorString(hipGetLastError()));
      return WMZ_ERR_HIP;
    }
  return WMZ_OK;
}
extern "C" int wmz_half_guard_clear(void* word, void* stream) {
  WMZ_REQUIRE(word != nullptr, "wmz_half_guard_clear: NULL word");
  if (hipMemsetAsync(word, 0, 4, (hipStream_t)stream) != hipSuccess) {
    wmz_set_error("wmz_half_guard_clear: %s", hipGetErrorString(hipGetLastError()));
    return WMZ_ERR_HIP;
  }
  return WMZ_OK;
}

namespace {

// x[b,s,h,w,:] = emb[z] + ((pos_s[s] + pos_h[h]) + pos_w[w])   (local_3d_attention.py:140-157)
// one 16-byte-wide lane per 4 channels; tables are fp32 and tiny (L2-resident), x is written once.
// The body of both kernels below.  PLANES: the launch computes the trailing rows_out rows of every clip's rows_in (whole planes):
// row `to` of x is the token grid's row t = fused_src_row(...) (fused_row_maps.h), whose token id and position indices it takes.
// The expression and its order are the whole grid's, so the planes produced are bit-identical to the whole grid's.
template <typename T, bool PLANES>
__device__ __forceinline__ void embed_pos3d_body(const int64_t* __restrict__ z, const float* __restrict__ emb,
                                                 const float* __restrict__ ps, const float* __restrict__ ph,
                                                 const float* __restrict__ pw, T* __restrict__ x, long ntok, int S, int H,
                                                 int W, int D, int num_classes, int rows_out, int rows_in, int row0) {
  const int d4 = D >> 2;
  const long total = ntok * d4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long to = i / d4;
    const int c = (int)(i - to * d4) * 4;
    const long t = PLANES ? fused_src_row(rows_out, rows_in, row0, to) : to;
    const int w = (int)(t % W);
    const int h = (int)((t / W) % H);
    const int s = (int)((t / ((long)W * H)) % S);
    long tok = z[t];
    tok = tok < 0 ? 0 : (tok >= num_classes ? num_classes - 1 : tok);   // reference would raise; stay in bounds
    const f32x4 e = *reinterpret_cast<const f32x4*>(emb + tok * D + c);
    const f32x4 a = *reinterpret_cast<const f32x4*>(ps + (long)s * D + c);
    const f32x4 bq = *reinterpret_cast<const f32x4*>(ph + (long)h * D + c);
    const f32x4 cw = *reinterpret_cast<const f32x4*>(pw + (long)w * D + c);
    const f32x4 v = e + ((a + bq) + cw);
    if constexpr (sizeof(T) == 4) {
      *reinterpret_cast<f32x4*>(x + to * D + c) = v;
    } else {
      s16x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = (short)f32_to_bf16_bits(v[k]);
      *reinterpret_cast<s16x4*>(x + to * D + c) = o;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void embed_pos3d_kernel(const int64_t* __restrict__ z, const float* __restrict__ emb,
                                                          const float* __restrict__ ps, const float* __restrict__ ph,
                                                          const float* __restrict__ pw, T* __restrict__ x, long ntok,
                                                          int S, int H, int W, int D, int num_classes) {
  embed_pos3d_body<T, false>(z, emb, ps, ph, pw, x, ntok, S, H, W, D, num_classes, 0, 0, 0);
}

// the trailing planes of every clip (wmz_embed_pos3d_fwd_planes): ntok = B planes_out H W rows of x
template <typename T>
__global__ __launch_bounds__(256) void embed_pos3d_planes_kernel(const int64_t* __restrict__ z, const float* __restrict__ emb,
                                                                 const float* __restrict__ ps, const float* __restrict__ ph,
                                                                 const float* __restrict__ pw, T* __restrict__ x, long ntok,
                                                                 int S, int H, int W, int D, int num_classes, int rows_out,
                                                                 int rows_in, int row0) {
  embed_pos3d_body<T, true>(z, emb, ps, ph, pw, x, ntok, S, H, W, D, num_classes, rows_out, rows_in, row0);
}

// Backward: one workgroup per (b, s) plane, thread = channel.  pos_s gets one row add per plane, pos_h / pos_w are
// reduced over the plane in LDS first (they would otherwise take B*S*W adds per element on a handful of rows);
// the token table takes one atomic row add per token.
template <typename T>
__global__ __launch_bounds__(256) void embed_pos3d_bwd_kernel(const int64_t* __restrict__ z, const T* __restrict__ dx,
                                                              float* __restrict__ demb, float* __restrict__ dps,
                                                              float* __restrict__ dph, float* __restrict__ dpw, int S,
                                                              int H, int W, int D, int num_classes) {
  extern __shared__ float sm[];     // [H][256] then [W][256]
  float* sh = sm;
  float* sw = sm + H * 256;
  const int plane = blockIdx.x;
  const int s = plane % S;
  const int t = threadIdx.x;
  for (int d0 = 0; d0 < D; d0 += 256) {
    const int d = d0 + t;
    for (int i = 0; i < H; ++i) sh[i * 256 + t] = 0.f;
    for (int i = 0; i < W; ++i) sw[i * 256 + t] = 0.f;
    float as = 0.f;
    // the LAST class is the denoiser's mask token (main.py:27: the embedding has num_embeddings + 1 rows): in the corrupted
    // frame about every other token carries it, and a thousand same-address atomics per element serialise in L2 -- its row
    // is summed per workgroup first (any other class sees ~64 adds per element, spread over the launch)
    float amask = 0.f;
    if (d < D) {
      for (int h = 0; h < H; ++h)
        for (int w = 0; w < W; ++w) {
          const long tok_i = ((long)plane * H + h) * W + w;
          const float v = Elem<T>::to_f32(dx[tok_i * D + d]);
          long tok = z[tok_i];
          tok = tok < 0 ? 0 : (tok >= num_classes ? num_classes - 1 : tok);
          if (tok == num_classes - 1) amask += v;
          else atomicAdd(demb + tok * D + d, v);
          as += v;
          sh[h * 256 + t] += v;
          sw[w * 256 + t] += v;
        }
      if (amask != 0.f) atomicAdd(demb + (long)(num_classes - 1) * D + d, amask);
      atomicAdd(dps + (long)s * D + d, as);
      for (int h = 0; h < H; ++h) atomicAdd(dph + (long)h * D + d, sh[h * 256 + t]);
      for (int w = 0; w < W; ++w) atomicAdd(dpw + (long)w * D + d, sw[w * 256 + t]);
    }
  }
}

// The same for W == 16 (the reference's latent planes): the per-column sums live in 16 registers and the per-row sum in
// one (the general kernel keeps both in LDS and every token pays two dependent LDS read-modify-writes, ~300 cycles of its
// ~430), the token ids of a plane row arrive by one load and are handed out by v_readlane, the row's 16 dx loads are
// independent and in flight together.
// PRECONDITION (embed_bwd16_takes below): the ids are loaded inside the `d < D` guard and read back from lanes 0..15, so every wave
// that enters the loop must have those lanes active: D % 64 is 0 or at least 16.  A narrower last wave (D % 64 in 1..15) would
// read ids from lanes that never executed the load and use them, unclamped, as a row of demb: such widths take the general kernel.
template <typename T>
__global__ __launch_bounds__(256) void embed_pos3d_bwd16_kernel(const int64_t* __restrict__ z, const T* __restrict__ dx,
                                                                float* __restrict__ demb, float* __restrict__ dps,
                                                                float* __restrict__ dph, float* __restrict__ dpw, int S,
                                                                int H, int D, int num_classes) {
  const int plane = blockIdx.x;
  const int s = plane % S;
  const int lane = threadIdx.x & 63;
  for (int d = threadIdx.x; d < D; d += 256) {
    float aw[16];
#pragma unroll
    for (int w = 0; w < 16; ++w) aw[w] = 0.f;
    float as = 0.f, amask = 0.f;
    for (int h = 0; h < H; ++h) {
      const long row = ((long)plane * H + h) * 16;
      long tk = z[row + (lane & 15)];                                     // this row's 16 token ids, one per lane (mod 16)
      tk = tk < 0 ? 0 : (tk >= num_classes ? num_classes - 1 : tk);
      const int tki = (int)tk;
      float v[16];
#pragma unroll
      for (int w = 0; w < 16; ++w) v[w] = Elem<T>::to_f32(dx[(row + w) * D + d]);
      float ah = 0.f;
#pragma unroll
      for (int w = 0; w < 16; ++w) {
        const int tok = __builtin_amdgcn_readlane(tki, w);
        if (tok == num_classes - 1) amask += v[w];                        // the mask token's row: summed per workgroup first
        else atomicAdd(demb + (long)tok * D + d, v[w]);
        aw[w] += v[w];
        ah += v[w];
      }
      as += ah;
      atomicAdd(dph + (long)h * D + d, ah);
    }
    if (amask != 0.f) atomicAdd(demb + (long)(num_classes - 1) * D + d, amask);
    atomicAdd(dps + (long)s * D + d, as);
#pragma unroll
    for (int w = 0; w < 16; ++w) atomicAdd(dpw + (long)w * D + d, aw[w]);
  }
}
// the shapes embed_pos3d_bwd16_kernel is launched for: its precondition above
static bool embed_bwd16_takes(int W, int D) { return W == 16 && (D % 64 == 0 || D % 64 >= 16); }

// config 5 (minecraft/sparse_diffusion.py:91-111): tokens at ARBITRARY flat grid positions `pos` (one per token):
// x[t,:] = emb[tok[t]] + ((pos_s[p / (H*W)] + pos_h[(p / W) % H]) + pos_w[p % W])
template <typename T>
__global__ __launch_bounds__(256) void embed_indexed_kernel(const int64_t* __restrict__ tok, const int64_t* __restrict__ pos,
                                                            const float* __restrict__ emb, const float* __restrict__ ps,
                                                            const float* __restrict__ ph, const float* __restrict__ pw,
                                                            T* __restrict__ x, long ntok, int S, int H, int W, int D,
                                                            int num_classes) {
  const int d4 = D >> 2;
  const long total = ntok * d4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long t = i / d4;
    const int c = (int)(i - t * d4) * 4;
    long p = pos[t];
    p = p < 0 ? 0 : (p >= (long)S * H * W ? (long)S * H * W - 1 : p);
    const int w = (int)(p % W), h = (int)((p / W) % H), s = (int)(p / ((long)W * H));
    long tk = tok[t];
    tk = tk < 0 ? 0 : (tk >= num_classes ? num_classes - 1 : tk);
    const f32x4 e = *reinterpret_cast<const f32x4*>(emb + tk * D + c);
    const f32x4 a = *reinterpret_cast<const f32x4*>(ps + (long)s * D + c);
    const f32x4 bq = *reinterpret_cast<const f32x4*>(ph + (long)h * D + c);
    const f32x4 cw = *reinterpret_cast<const f32x4*>(pw + (long)w * D + c);
    const f32x4 v = e + ((a + bq) + cw);
    if constexpr (sizeof(T) == 4) {
      *reinterpret_cast<f32x4*>(x + t * D + c) = v;
    } else {
      s16x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = (short)f32_to_bf16_bits(v[k]);
      *reinterpret_cast<s16x4*>(x + t * D + c) = o;
    }
  }
}

// Gradient of the indexed embedding sum (config 5: 3 072 tokens x 512 columns into 64 + 16 + 16 position rows and an 8 193-row token
// table of which ONE row, the mask token's, takes half the tokens).  Four global atomics per element (round 2) meant up to 1 536
// adds on one address: 57 us at the end of config 5's backward chain.  Here a workgroup owns a slab of EB_COLS columns and a group
// of tokens: the three position tables and the hot token row (the table's last: the mask token, main.py:27) are summed in LDS
// (ds_add_f32) and flushed once per workgroup -- 16 adds per address instead of 192 - 1 536 --, the other token rows go to memory
// directly (mostly distinct addresses).  Isolated: 57 -> 33 us; by ablation half of what is left is the LDS float atomics
// themselves (they retire at about a lane a clock), the rest zeroing, flush and index arithmetic.
constexpr int EB_COLS = 32;

template <typename T>
__global__ __launch_bounds__(256) void embed_indexed_bwd_kernel(const int64_t* __restrict__ tok, const int64_t* __restrict__ pos,
                                                                const T* __restrict__ dx, float* __restrict__ demb,
                                                                float* __restrict__ dps, float* __restrict__ dph,
                                                                float* __restrict__ dpw, long ntok, int S, int H, int W,
                                                                int D, int num_classes, int tgroups, int use_lds) {
  extern __shared__ float tab[];                              // [(S + H + W + 1) rows][EB_COLS]; use_lds == 0 (tables beyond the LDS): all to memory
  const int nrows = S + H + W + 1;
  const int slab = blockIdx.x / tgroups, tg = blockIdx.x - slab * tgroups;
  const int d0 = slab * EB_COLS;
  const int col = threadIdx.x & (EB_COLS - 1), trow = threadIdx.x / EB_COLS;            // 8 tokens per sweep
  if (use_lds)
    for (int i = threadIdx.x; i < nrows * EB_COLS; i += 256) tab[i] = 0.f;
  __syncthreads();
  const int d = d0 + col;
  const long per = (ntok + tgroups - 1) / tgroups;
  const long t0 = (long)tg * per, t1 = t0 + per < ntok ? t0 + per : ntok;
  if (d < D) {
    // four tokens of the thread at a time: their loads are issued together (one token per trip made the loop a chain of load
    // latencies: 59 us at 384 tokens a workgroup), indices in 32-bit arithmetic
    constexpr int TS = 256 / EB_COLS, UN = 4;
    const int HW = H * W, G = S * HW;
    for (long tb = t0 + trow; tb < t1; tb += TS * UN) {
      int pi[UN], ti[UN];
      float v[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const long t = tb + (long)u * TS;
        const bool in = t < t1;
        const long tt = in ? t : t1 - 1;
        const long p = pos[tt], tk = tok[tt];
        pi[u] = p < 0 ? 0 : (p >= G ? G - 1 : (int)p);
        ti[u] = in ? (tk < 0 ? 0 : (tk >= num_classes ? num_classes - 1 : (int)tk)) : -1;
        v[u] = Elem<T>::to_f32(dx[tt * D + d]);
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        if (ti[u] < 0) continue;
        const int sI = pi[u] / HW, rem = pi[u] - sI * HW, h = rem / W, w = rem - h * W;
        if (use_lds) {
          atomicAdd(&tab[sI * EB_COLS + col], v[u]);
          atomicAdd(&tab[(S + h) * EB_COLS + col], v[u]);
          atomicAdd(&tab[(S + H + w) * EB_COLS + col], v[u]);
          if (ti[u] == num_classes - 1) atomicAdd(&tab[(S + H + W) * EB_COLS + col], v[u]);
          else atomicAdd(demb + (long)ti[u] * D + d, v[u]);
        } else {
          atomicAdd(dps + (long)sI * D + d, v[u]);
          atomicAdd(dph + (long)h * D + d, v[u]);
          atomicAdd(dpw + (long)w * D + d, v[u]);
          atomicAdd(demb + (long)ti[u] * D + d, v[u]);
        }
      }
    }
  }
  __syncthreads();
  if (!use_lds) return;
  for (int i = threadIdx.x; i < nrows * EB_COLS; i += 256) {
    const int r = i / EB_COLS, c = d0 + (i - r * EB_COLS);
    const float v = tab[i];
    if (c >= D || v == 0.f) continue;
    if (r < S) atomicAdd(dps + (long)r * D + c, v);
    else if (r < S + H) atomicAdd(dph + (long)(r - S) * D + c, v);
    else if (r < S + H + W) atomicAdd(dpw + (long)(r - S - H) * D + c, v);
    else atomicAdd(demb + (long)(num_classes - 1) * D + c, v);
  }
}

}  // namespace

extern "C" int wmz_embed_indexed_fwd(const int64_t* tok, const int64_t* pos, const float* emb, const float* pos_s,
                                     const float* pos_h, const float* pos_w, void* x, long ntok, int S, int H, int W,
                                     int D, int num_classes, int dtype, void* stream) {
  WMZ_REQUIRE(tok && pos && emb && pos_s && pos_h && pos_w && x, "wmz_embed_indexed_fwd: null tensor");
  WMZ_REQUIRE(ntok > 0 && S > 0 && H > 0 && W > 0 && D > 0 && D % 4 == 0 && num_classes > 0, "wmz_embed_indexed_fwd: bad shape");
  WMZ_REQUIRE(dtype == WMZ_F32 || dtype == WMZ_BF16, "wmz_embed_indexed_fwd: bad dtype %d", dtype);
  const long total = ntok * (D / 4);
  const int grid = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == WMZ_BF16)
    hipLaunchKernelGGL(embed_indexed_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, tok, pos, emb, pos_s, pos_h, pos_w, (bf16_t*)x, ntok, S, H, W, D, num_classes);
  else
    hipLaunchKernelGGL(embed_indexed_kernel<float>, dim3(grid), dim3(256), 0, st, tok, pos, emb, pos_s, pos_h, pos_w, (float*)x, ntok, S, H, W, D, num_classes);
  WMZ_LAUNCH_CHECK("wmz_embed_indexed_fwd");
  return WMZ_OK;
}

extern "C" int wmz_embed_indexed_bwd(const int64_t* tok, const int64_t* pos, const void* dx, float* demb, float* dpos_s,
                                     float* dpos_h, float* dpos_w, long ntok, int S, int H, int W, int D, int num_classes,
                                     int dtype, void* stream) {
  WMZ_REQUIRE(tok && pos && dx && demb && dpos_s && dpos_h && dpos_w, "wmz_embed_indexed_bwd: null tensor");
  WMZ_REQUIRE(ntok > 0 && S > 0 && H > 0 && W > 0 && D > 0 && num_classes > 0, "wmz_embed_indexed_bwd: bad shape");
  WMZ_REQUIRE(dtype == WMZ_F32 || dtype == WMZ_BF16, "wmz_embed_indexed_bwd: bad dtype %d", dtype);
  const int slabs = (D + EB_COLS - 1) / EB_COLS;
  size_t lds = (size_t)(S + H + W + 1) * EB_COLS * sizeof(float);
  const int use_lds = lds <= 60 * 1024;
  if (!use_lds) lds = 0;
  // token groups: enough workgroups to fill the chip, at least 64 tokens each
  int tgroups = 512 / slabs;
  if (tgroups < 1) tgroups = 1;
  while (tgroups > 1 && ntok / tgroups < 64) tgroups >>= 1;
  const int grid = slabs * tgroups;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == WMZ_BF16)
    hipLaunchKernelGGL(embed_indexed_bwd_kernel<bf16_t>, dim3(grid), dim3(256), lds, st, tok, pos, (const bf16_t*)dx, demb, dpos_s, dpos_h, dpos_w, ntok, S, H, W, D, num_classes, tgroups, use_lds);
  else
    hipLaunchKernelGGL(embed_indexed_bwd_kernel<float>, dim3(grid), dim3(256), lds, st, tok, pos, (const float*)dx, demb, dpos_s, dpos_h, dpos_w, ntok, S, H, W, D, num_classes, tgroups, use_lds);
  WMZ_LAUNCH_CHECK("wmz_embed_indexed_bwd");
  return WMZ_OK;
}

extern "C" int wmz_embed_pos3d_bwd(const int64_t* z, const void* dx, float* demb, float* dpos_s, float* dpos_h,
                                   float* dpos_w, int B, int S, int H, int W, int D, int num_classes, int dtype,
                                   void* stream) {
  WMZ_REQUIRE(z && dx && demb && dpos_s && dpos_h && dpos_w, "wmz_embed_pos3d_bwd: null tensor");
  WMZ_REQUIRE(B > 0 && S > 0 && H > 0 && W > 0 && D > 0 && num_classes > 0, "wmz_embed_pos3d_bwd: bad shape");
  WMZ_REQUIRE(dtype == WMZ_F32 || dtype == WMZ_BF16, "wmz_embed_pos3d_bwd: bad dtype %d", dtype);
  const size_t smem = (size_t)(H + W) * 256 * sizeof(float);
  if (smem > 64 * 1024) { wmz_set_error("wmz_embed_pos3d_bwd: H + W = %d > 64 not built", H + W); return WMZ_ERR_UNSUPPORTED; }
  hipStream_t st = (hipStream_t)stream;
  if (embed_bwd16_takes(W, D)) {
    if (dtype == WMZ_BF16)
      hipLaunchKernelGGL(embed_pos3d_bwd16_kernel<bf16_t>, dim3(B * S), dim3(256), 0, st, z, (const bf16_t*)dx, demb, dpos_s, dpos_h,
                         dpos_w, S, H, D, num_classes);
    else
      hipLaunchKernelGGL(embed_pos3d_bwd16_kernel<float>, dim3(B * S), dim3(256), 0, st, z, (const float*)dx, demb, dpos_s, dpos_h,
                         dpos_w, S, H, D, num_classes);
    WMZ_LAUNCH_CHECK("wmz_embed_pos3d_bwd");
    return WMZ_OK;
  }
  if (dtype == WMZ_BF16)
    hipLaunchKernelGGL(embed_pos3d_bwd_kernel<bf16_t>, dim3(B * S), dim3(256), smem, st, z, (const bf16_t*)dx, demb, dpos_s,
                       dpos_h, dpos_w, S, H, W, D, num_classes);
  else
    hipLaunchKernelGGL(embed_pos3d_bwd_kernel<float>, dim3(B * S), dim3(256), smem, st, z, (const float*)dx, demb, dpos_s,
                       dpos_h, dpos_w, S, H, W, D, num_classes);
  WMZ_LAUNCH_CHECK("wmz_embed_pos3d_bwd");
  return WMZ_OK;
}

extern "C" int wmz_embed_pos3d_fwd(const int64_t* z, const float* emb, const float* pos_s, const float* pos_h,
                                   const float* pos_w, void* x, int B, int S, int H, int W, int D, int num_classes,
                                   int dtype, void* stream) {
  WMZ_REQUIRE(z && emb && pos_s && pos_h && pos_w && x, "wmz_embed_pos3d_fwd: null tensor");
  WMZ_REQUIRE(B > 0 && S > 0 && H > 0 && W > 0 && D > 0 && num_classes > 0, "wmz_embed_pos3d_fwd: bad shape");
  WMZ_REQUIRE(D % 4 == 0, "wmz_embed_pos3d_fwd: D must be a multiple of 4 (got %d)", D);
  WMZ_REQUIRE(dtype == WMZ_F32 || dtype == WMZ_BF16, "wmz_embed_pos3d_fwd: bad dtype %d", dtype);
  const long ntok = (long)B * S * H * W;
  const long total = ntok * (D / 4);
  const int grid = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == WMZ_BF16)
    hipLaunchKernelGGL(embed_pos3d_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, z, emb, pos_s, pos_h, pos_w,
                       (bf16_t*)x, ntok, S, H, W, D, num_classes);
  else
    hipLaunchKernelGGL(embed_pos3d_kernel<float>, dim3(grid), dim3(256), 0, st, z, emb, pos_s, pos_h, pos_w,
                       (float*)x, ntok, S, H, W, D, num_classes);
  WMZ_LAUNCH_CHECK("wmz_embed_pos3d_fwd");
  return WMZ_OK;
}

// The trailing planes_out planes of the same embedding: x [B, planes_out, H, W, D], every element by the expression above
// (embed_pos3d_body), bit-identical to those planes of wmz_embed_pos3d_fwd.  planes_out == S is that launch's result.
extern "C" int wmz_embed_pos3d_fwd_planes(const int64_t* z, const float* emb, const float* pos_s, const float* pos_h,
                                          const float* pos_w, void* x, int B, int S, int H, int W, int planes_out, int D,
                                          int num_classes, int dtype, void* stream) {
  WMZ_REQUIRE(z && emb && pos_s && pos_h && pos_w && x, "wmz_embed_pos3d_fwd_planes: null tensor");
  WMZ_REQUIRE(B > 0 && S > 0 && H > 0 && W > 0 && D > 0 && num_classes > 0, "wmz_embed_pos3d_fwd_planes: bad shape");
  WMZ_REQUIRE(planes_out > 0 && planes_out <= S, "wmz_embed_pos3d_fwd_planes: bad plane count");
  WMZ_REQUIRE(D % 4 == 0, "wmz_embed_pos3d_fwd_planes: D must be a multiple of 4 (got %d)", D);
  WMZ_REQUIRE(dtype == WMZ_F32 || dtype == WMZ_BF16, "wmz_embed_pos3d_fwd_planes: bad dtype %d", dtype);
  WMZ_REQUIRE((long)B * S * H * W < (1L << 31), "wmz_embed_pos3d_fwd_planes: token count overflows int");
  const int HW = H * W;
  const long ntok = (long)B * planes_out * HW;
  const long total = ntok * (D / 4);
  const int grid = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == WMZ_BF16)
    hipLaunchKernelGGL(embed_pos3d_planes_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, z, emb, pos_s, pos_h, pos_w,
                       (bf16_t*)x, ntok, S, H, W, D, num_classes, planes_out * HW, S * HW, (S - planes_out) * HW);
  else
    hipLaunchKernelGGL(embed_pos3d_planes_kernel<float>, dim3(grid), dim3(256), 0, st, z, emb, pos_s, pos_h, pos_w,
                       (float*)x, ntok, S, H, W, D, num_classes, planes_out * HW, S * HW, (S - planes_out) * HW);
  WMZ_LAUNCH_CHECK("wmz_embed_pos3d_fwd_planes");
  return WMZ_OK;
}

// ---- development probe (csrc/wmz_debug.h): a wall-clock marker between the phases of a captured step
namespace {
__global__ void stamp_kernel(long long* buf, int slot) { buf[slot] = (long long)wall_clock64(); }
}  // namespace
extern "C" int wmz_debug_stamp(void* buf, int slot, void* stream) {
  WMZ_REQUIRE(buf != nullptr && slot >= 0, "wmz_debug_stamp: bad arguments");
  hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (long long*)buf, slot);
  WMZ_LAUNCH_CHECK("wmz_debug_stamp");
  return WMZ_OK;
}
