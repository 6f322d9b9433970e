// Attention pool of SimpleAttention / MatchingAttention (model/DialogueRNN.py:6-77) as standalone modules: score, softmax and pool
// stages and their backward (include/mser.h "Attention pool").  Each pass is three launches, so that a batch of B rows fills the chip
// rather than B workgroups:
//   rows   one wave per memory row (j, b): the raw score (forward) or g = dpool . M_j + dalpha (backward); S*B rows, 4 per workgroup;
//   norm   one workgroup per batch row: softmax over the S entries of the row in place (the 'general2' mask and renormalisation), or
//          its backward ds = alpha (g - sum alpha g) (* mask); every entry is read and written by the thread that owns it;
//   cols   one wave per (64 features, b): pool / dM and dq, or the 'concat' dA / dxb / dvb, walking the S rows of that b.
#include "common.h"
#include "../../include/mser.h"

using namespace mser;

namespace {

constexpr int AP_WAVES = 4;
constexpr int AP_THREADS = 64 * AP_WAVES;

template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float* red) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  v = MAX ? wave_max(v) : wave_sum(v);
  __syncthreads();                       // red may still be read by the previous reduction
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int w = 1; w < AP_WAVES; ++w) r = MAX ? fmaxf(r, red[w]) : r + red[w];
  return r;
}

__device__ __forceinline__ float mask_of(const mser_attn_pool_desc& d, int b, int j) {
  return (d.type == MSER_ATT_GENERAL2 && d.mask) ? d.mask[(long)b * d.S + j] : 1.f;
}

// ---- rows: one wave per (j, b), row r = j*B + b --------------------------------------------------------------------------------
template <bool BWD>
__global__ __launch_bounds__(AP_THREADS) void attn_pool_rows_kernel(mser_attn_pool_desc d) {
  const long r = (long)blockIdx.x * AP_WAVES + (threadIdx.x >> 6);
  if (r >= (long)d.S * d.B) return;
  const int lane = threadIdx.x & 63;
  const int j = (int)(r / d.B), b = (int)(r % d.B);
  float acc = 0.f;
  if (!BWD && d.type == MSER_ATT_CONCAT) {
    const float* a = d.A + r * d.lda;
    const float* xb = d.xb + (long)b * d.Da;
    for (int k = lane; k < d.Da; k += 64) acc = fmaf(d.v[k], tanhf(a[k] + xb[k]), acc);
  } else {
    const float* m = d.M + (long)j * d.sMj + (long)b * d.sMb;
    const float* q = BWD ? d.dpool + (long)b * d.D : d.q + (long)b * d.sqb;
    for (int k = lane; k < d.D; k += 64) acc = fmaf(q[k], m[k], acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    if (BWD) d.ds[(long)b * d.S + j] = acc + (d.dalpha ? d.dalpha[(long)b * d.S + j] : 0.f);
    else d.alpha[(long)b * d.S + j] = acc * mask_of(d, b, j);       // GENERAL2 masks the logits (:64)
  }
}

// ---- norm: one workgroup per batch row ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(AP_THREADS) void attn_pool_softmax_kernel(mser_attn_pool_desc d) {
  __shared__ float red[AP_WAVES];
  const int b = blockIdx.x, S = d.S;
  float* al = d.alpha + (long)b * S;
  float mx = -INFINITY;
  for (int j = threadIdx.x; j < S; j += AP_THREADS) mx = fmaxf(mx, al[j]);
  mx = block_reduce<true>(mx, red);
  // softmax; GENERAL2 then masks and renormalises: alpha = e m / sum(e m) (the softmax denominator cancels)
  float z = 0.f;
  for (int j = threadIdx.x; j < S; j += AP_THREADS) {
    const float e = expf(al[j] - mx) * mask_of(d, b, j);
    al[j] = e;
    z += e;
  }
  z = block_reduce<false>(z, red);
  const float inv = 1.f / z;
  for (int j = threadIdx.x; j < S; j += AP_THREADS) al[j] *= inv;
}

__global__ __launch_bounds__(AP_THREADS) void attn_pool_softmax_bwd_kernel(mser_attn_pool_desc d) {
  __shared__ float red[AP_WAVES];
  const int b = blockIdx.x, S = d.S;
  const float* al = d.alpha + (long)b * S;
  float* ds = d.ds + (long)b * S;
  float dot = 0.f;
  for (int j = threadIdx.x; j < S; j += AP_THREADS) dot = fmaf(al[j], ds[j], dot);
  dot = block_reduce<false>(dot, red);
  // d score: alpha (g - sum alpha g); GENERAL2 (alpha = e m / sum e m over the logits s m): the same, times m
  for (int j = threadIdx.x; j < S; j += AP_THREADS) ds[j] = al[j] * (ds[j] - dot) * mask_of(d, b, j);
}

// ---- cols: one wave per (64 features, b) --------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void attn_pool_pool_kernel(mser_attn_pool_desc d) {
  const int k = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
  if (k >= d.D) return;
  const float* al = d.alpha + (long)b * d.S;
  const float* mb = d.M + (long)b * d.sMb + k;
  float acc = 0.f;
  for (int j = 0; j < d.S; ++j) acc = fmaf(al[j], mb[(long)j * d.sMj], acc);
  d.pool[(long)b * d.D + k] = acc;
}

__global__ __launch_bounds__(64) void attn_pool_dm_kernel(mser_attn_pool_desc d) {
  const int k = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
  if (k >= d.D) return;
  const int S = d.S, B = d.B, D = d.D;
  const float* al = d.alpha + (long)b * S;
  const float* ds = d.ds + (long)b * S;
  const float pk = d.dpool[(long)b * D + k];
  if (d.type == MSER_ATT_CONCAT) {          // the score side reaches M through W_M: the caller adds dA W_M
    for (int j = 0; j < S; ++j) d.dM[((long)j * B + b) * D + k] = al[j] * pk;
    return;
  }
  const float qk = d.q[(long)b * d.sqb + k];
  const float* mb = d.M + (long)b * d.sMb + k;
  float acc = 0.f;
  for (int j = 0; j < S; ++j) {
    acc = fmaf(ds[j], mb[(long)j * d.sMj], acc);
    d.dM[((long)j * B + b) * D + k] = fmaf(ds[j], qk, al[j] * pk);
  }
  d.dq[(long)b * D + k] = acc;
}

__global__ __launch_bounds__(64) void attn_pool_concat_bwd_kernel(mser_attn_pool_desc d) {
  const int k = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
  if (k >= d.Da) return;
  const int S = d.S, B = d.B;
  const float* ds = d.ds + (long)b * S;
  const float xk = d.xb[(long)b * d.Da + k], vk = d.v[k];
  float accx = 0.f, accv = 0.f;
  for (int j = 0; j < S; ++j) {
    const long r = ((long)j * B + b) * d.lda + k;
    const float t = tanhf(d.A[r] + xk);
    const float g = ds[j] * vk * (1.f - t * t);
    d.dA[r] = g;
    accx += g;
    accv = fmaf(ds[j], t, accv);
  }
  d.dxb[(long)b * d.Da + k] = accx;
  d.dvb[(long)b * d.Da + k] = accv;
}

int check_desc(const mser_attn_pool_desc* d, const char* what) {
  MSER_REQUIRE(d, "%s: null descriptor", what);
  MSER_REQUIRE(d->type >= MSER_ATT_SIMPLE && d->type <= MSER_ATT_CONCAT, "%s: unknown type %d", what, d->type);
  MSER_REQUIRE(d->S >= 1 && d->S <= MSER_ATTN_POOL_MAX_S, "%s: S = %d outside [1, %d] (an empty memory is the caller's case)", what,
               d->S, MSER_ATTN_POOL_MAX_S);
  MSER_REQUIRE(d->B >= 0 && d->B <= 65535 && d->D >= 1 && d->M && d->alpha, "%s: bad sizes or pointers", what);
  if (d->type == MSER_ATT_CONCAT)
    MSER_REQUIRE(d->Da >= 1 && d->A && d->xb && d->v && d->lda >= d->Da, "%s: CONCAT needs Da, A, xb, v", what);
  else
    MSER_REQUIRE(d->q, "%s: the score query q is missing", what);
  return 0;
}

}  // namespace

extern "C" {

int mser_attn_pool_fwd(const mser_attn_pool_desc* d, mser_stream_t stream) {
  MSER_TRY(check_desc(d, "mser_attn_pool_fwd"));
  MSER_REQUIRE(d->pool, "mser_attn_pool_fwd: pool is missing");
  if (d->B == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(attn_pool_rows_kernel<false>, dim3(cdiv((long)d->S * d->B, AP_WAVES)), dim3(AP_THREADS), 0, s, *d);
  hipLaunchKernelGGL(attn_pool_softmax_kernel, dim3(d->B), dim3(AP_THREADS), 0, s, *d);
  hipLaunchKernelGGL(attn_pool_pool_kernel, dim3(cdiv(d->D, 64), d->B), dim3(64), 0, s, *d);
  return check_launch("mser_attn_pool_fwd");
}

int mser_attn_pool_bwd(const mser_attn_pool_desc* d, mser_stream_t stream) {
  MSER_TRY(check_desc(d, "mser_attn_pool_bwd"));
  MSER_REQUIRE(d->dpool && d->dM && d->ds, "mser_attn_pool_bwd: dpool / dM / ds missing");
  if (d->type == MSER_ATT_CONCAT)
    MSER_REQUIRE(d->dA && d->dxb && d->dvb, "mser_attn_pool_bwd: CONCAT needs dA, dxb, dvb");
  else
    MSER_REQUIRE(d->dq, "mser_attn_pool_bwd: dq missing");
  if (d->B == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(attn_pool_rows_kernel<true>, dim3(cdiv((long)d->S * d->B, AP_WAVES)), dim3(AP_THREADS), 0, s, *d);
  hipLaunchKernelGGL(attn_pool_softmax_bwd_kernel, dim3(d->B), dim3(AP_THREADS), 0, s, *d);
  hipLaunchKernelGGL(attn_pool_dm_kernel, dim3(cdiv(d->D, 64), d->B), dim3(64), 0, s, *d);
  if (d->type == MSER_ATT_CONCAT)
    hipLaunchKernelGGL(attn_pool_concat_bwd_kernel, dim3(cdiv(d->Da, 64), d->B), dim3(64), 0, s, *d);
  return check_launch("mser_attn_pool_bwd");
}

}  // extern "C"
