// racinglmpc_amd/csrc/lmpc_noise.hip.h -- counter-based N(0, 1) draws generated on the device: the plant disturbance of a rollout session (stream 0) and the
// control-law noise of a PID lap (stream 1) without a host draw or an upload.  The reference has no counterpart beyond np.random.randn() at SysModel.py:139-141
// and Utilities.py:67-68.  Included by lmpc_capi.hip only (the variant libraries carry no noise kernel).
//
// The draw for (seed, stream, lap, t, car) is a pure function of those five numbers:
//   block function   Philox4x64-10 as NumPy's Philox bit generator implements it -- the four words are what
//                    numpy.random.Philox(counter=[t, car, lap, stream], key=[seed, 0]).random_raw(4) returns.  NumPy increments word 0 of the counter before
//                    its first block, so the block function is evaluated on the counter [t + 1, car, lap, stream] with the key [seed, 0].
//   transform        Box-Muller in FP64 on the word pairs (w0, w1) and (w2, w3): u1 = ((w0 >> 11) + 1) 2^-53 in (0, 1], u2 = (w1 >> 11) 2^-53 in [0, 1),
//                    r = sqrt(-2 log u1), z0 = r cos(2 pi u2), z1 = r sin(2 pi u2); z2, z3 likewise.  Width 3 (plant) stores z0, z1, z2; width 2 (control law)
//                    stores z0, z1 and never evaluates the second pair.
// The library is built without fast-math options: log, sin and cos below are the ocml double-precision functions, sqrt the correctly rounded one.
#pragma once
#include <hip/hip_runtime.h>

#define LMPC_NOISE_NT 256                      // threads per work-group of the two kernels below: one thread per (t, car)

struct lmpc_philox_words { unsigned long long w[4]; };

// Philox4x64-10.  Round: c' = [hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)]; the key is bumped by the Weyl constants after every round.
__device__ __forceinline__ lmpc_philox_words lmpc_philox4x64_10(unsigned long long c0, unsigned long long c1, unsigned long long c2, unsigned long long c3,
                                                                 unsigned long long k0, unsigned long long k1) {
    const unsigned long long M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull, W0 = 0x9E3779B97F4A7C15ull, W1 = 0xBB67AE8584CAA73Bull;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned long long hi0 = __umul64hi(M0, c0), lo0 = M0 * c0, hi1 = __umul64hi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += W0; k1 += W1;
    }
    lmpc_philox_words o; o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
    return o;
}

// the four words of (seed, stream, lap, t, car): NumPy's first block of counter [t, car, lap, stream] is the block function at t + 1
__device__ __forceinline__ lmpc_philox_words lmpc_noise_words(unsigned long long seed, unsigned long long stream, unsigned long long lap, unsigned long long t, unsigned long long car) {
    return lmpc_philox4x64_10(t + 1ull, car, lap, stream, seed, 0ull);
}

__device__ __forceinline__ void lmpc_box_muller(unsigned long long wa, unsigned long long wb, double &za, double &zb) {
#pragma clang fp contract(off)
    const double u1 = (double)((wa >> 11) + 1ull) * 0x1.0p-53;      // (0, 1]: at most 2^53, exact in FP64
    const double u2 = (double)(wb >> 11) * 0x1.0p-53;               // [0, 1)
    const double r = sqrt(-2.0 * log(u1));
    const double a = 6.283185307179586 * u2;                        // 2 pi rounded to FP64 (0x401921FB54442D18)
    za = r * cos(a); zb = r * sin(a);
}

// out[((t - t0) B + b) width + j], j < width: the layout lmpc_rollout_plant_kernel / lmpc_pid_rollout_kernel index (T x B x 3, T x B x 2).  One thread per (t, car);
// size_t indexing throughout (T_max x B x width passes 2^31 elements at 100000 steps x 8192 cars).
__global__ void __launch_bounds__(LMPC_NOISE_NT) lmpc_noise_fill_kernel(unsigned long long seed, unsigned long long stream, unsigned long long lap, unsigned long long t0,
                                                                        int T, unsigned long long car0, int B, int width, double *__restrict__ out) {
    const size_t e = (size_t)blockIdx.x * LMPC_NOISE_NT + threadIdx.x, total = (size_t)T * (size_t)B;
    if (e >= total) return;
    const size_t tr = e / (size_t)B, b = e - tr * (size_t)B;
    const lmpc_philox_words w = lmpc_noise_words(seed, stream, lap, t0 + tr, car0 + b);
    double z0, z1;
    lmpc_box_muller(w.w[0], w.w[1], z0, z1);
    double *o = out + e * (size_t)width;
    o[0] = z0; o[1] = z1;
    if (width == 3) { double z2, z3; lmpc_box_muller(w.w[2], w.w[3], z2, z3); o[2] = z2; }
}

// words[((t - t0) B + b) 4 + j]: the four raw words of each (t, car) and nothing else (the bit-exact check of the block function and its addressing against NumPy)
__global__ void __launch_bounds__(LMPC_NOISE_NT) lmpc_noise_raw_kernel(unsigned long long seed, unsigned long long stream, unsigned long long lap, unsigned long long t0,
                                                                       int T, unsigned long long car0, int B, unsigned long long *__restrict__ words) {
    const size_t e = (size_t)blockIdx.x * LMPC_NOISE_NT + threadIdx.x, total = (size_t)T * (size_t)B;
    if (e >= total) return;
    const size_t tr = e / (size_t)B, b = e - tr * (size_t)B;
    const lmpc_philox_words w = lmpc_noise_words(seed, stream, lap, t0 + tr, car0 + b);
    unsigned long long *o = words + e * 4;
    o[0] = w.w[0]; o[1] = w.w[1]; o[2] = w.w[2]; o[3] = w.w[3];
}

// launch of the fill on `st`; the grid holds ceil(T B / 256) work-groups (the callers bound T B so that it fits a grid dimension)
static inline void lmpc_noise_fill_launch(hipStream_t st, unsigned long long seed, unsigned long long stream, unsigned long long lap, long long t0, int T, long long car0, int B,
                                          int width, double *out_dev) {
    const size_t total = (size_t)T * (size_t)B;
    hipLaunchKernelGGL(lmpc_noise_fill_kernel, dim3((unsigned)((total + LMPC_NOISE_NT - 1) / LMPC_NOISE_NT)), dim3(LMPC_NOISE_NT), 0, st, seed, stream, lap,
                       (unsigned long long)t0, T, (unsigned long long)car0, B, width, out_dev);
}
