// The dropout stream's two entry points (dropout.h defines the stream): the
// key kernel that opens every forward with dropout, and the mask written out
// with the device function the kernels use.
#include "common.h"

namespace {

// key_out = (seed, counter); counter += 1.  One thread: a replayed HIP graph
// advances the counter with no host involvement.
__global__ void k_dropout_next_key(int64_t* __restrict__ state, int64_t* __restrict__ key_out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int64_t seed = state[0], n = state[1];
  key_out[0] = seed;
  key_out[1] = n;
  state[1] = n + 1;
}

__global__ __launch_bounds__(256) void k_dropout_mask(DropArgs dr, uint8_t* __restrict__ keep,
                                                      int64_t N, int d4) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N * d4) return;
  const int64_t i = t / d4;
  const int c = (int)(t - i * d4);
  const uint4 w = Drop<DropArgs>(dr).words(i, c);
  reinterpret_cast<uchar4*>(keep)[t] =
      make_uchar4(w.x >= dr.thr, w.y >= dr.thr, w.z >= dr.thr, w.w >= dr.thr);
}

}  // namespace

MOLCLR_API int molclr_dropout_next_key(int64_t* state, int64_t* key_out, molclr_stream_t stream) {
  MOLCLR_REQUIRE(state && key_out && state != key_out, "dropout_next_key: null or aliased pointer");
  hipLaunchKernelGGL(k_dropout_next_key, dim3(1), dim3(1), 0, molclr::as_stream(stream), state,
                     key_out);
  MOLCLR_LAUNCHED();
  return MOLCLR_OK;
}

MOLCLR_API int molclr_dropout_mask(const int64_t* key, int layer, double p, uint8_t* keep,
                                   int64_t N, int64_t D, molclr_stream_t stream) {
  MOLCLR_REQUIRE(p >= 0.0 && p < 1.0, "dropout_mask: p %g outside [0, 1)", p);
  MOLCLR_REQUIRE(D > 0 && D % 4 == 0 && N >= 0, "dropout_mask: dim %lld must be a multiple of 4",
                 (long long)D);
  MOLCLR_REQUIRE(layer >= 0 && layer < MOLCLR_MAX_LAYERS, "dropout_mask: layer %d", layer);
  if (N == 0) return MOLCLR_OK;
  MOLCLR_REQUIRE(key && keep && ((uintptr_t)keep & 3) == 0,
                 "dropout_mask: null pointer or keep not 4-byte aligned");
  const int d4 = (int)(D / 4);
  hipLaunchKernelGGL(k_dropout_mask, dim3(molclr::ceil_div(N * d4, 256)), dim3(256), 0,
                     molclr::as_stream(stream), make_drop_args(key, p, layer), keep, N, d4);
  MOLCLR_LAUNCHED();
  return MOLCLR_OK;
}
