/*
 * npb_noise.hip -- the heat-source noise streams on the device: one Mersenne Twister per plant that follows
 * numpy.random.RandomState(seed).standard_normal() (the reference's ConstantHeatSource draws rng.normal(0, sigma) per step,
 * constant_heat_source.py:58-62,178; numpy's legacy normal is loc + scale * gauss).
 *
 * What is restated is numpy 2.2's published legacy path, as nuclear_sim_amd/csrc/npb_seeds.cpp does for the host: MT19937
 * (Matsumoto & Nishimura 1998) seeded by init_genrand, a word per call with the twist made when pos reaches 624, doubles from two
 * words ((a >> 5) * 2^26 + (b >> 6)) / 2^53, and legacy_gauss: the polar method with a one-value cache that is zeroed when consumed.
 *
 * Built on its own (Makefile): -ffp-contract=off keeps r2 = x1 * x1 + x2 * x2 two rounded products and one rounded sum, so every
 * accept / reject decision -- and with it the word stream -- is numpy's bit for bit; without -freciprocal-math / -fapprox-func the
 * division and the square root are IEEE, and only the device library's fp64 log can differ from the host's libm.
 *
 * One lane per plant.  Lanes reject independently and so run out of words at different draws; a lane that does waits, and the
 * wave twists every waiting lane in one pass, so the 624-word loop is run once per generation for the wave, not once per lane.
 *
 * The same generator, on a second set of states, feeds the data-gen runner's power profile: npb_profile_rows_kernel (below) turns a
 * block of its draws into target and setpoint rows, and has the ramp stage alone as a second entry.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include "npb_noise.h"

namespace {

constexpr int MT_N = NPB_MT_N, MT_M = 397;
constexpr uint32_t UPPER = 0x80000000u, LOWER = 0x7fffffffu, MATRIX_A = 0x9908b0dfu;

__device__ __forceinline__ uint32_t temper(uint32_t y) {
  y ^= (y >> 11);
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= (y >> 18);
  return y;
}

__device__ __forceinline__ uint32_t twist_word(uint32_t cur, uint32_t next, uint32_t far) {
  const uint32_t y = (cur & UPPER) | (next & LOWER);
  return far ^ (y >> 1) ^ ((y & 1u) ? MATRIX_A : 0u);
}

__device__ __forceinline__ double to_double(uint32_t a, uint32_t b) {
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) / 9007199254740992.0;
}

/* words [i, hi) of the twist, B at a time, word j from words j, j + 1 and j + off: each batch issues all its loads before its
 * stores.  No batch reads a word it writes: for j < 227 the far word j + 397 is not written in this pass, for 227 <= j < 623 it is
 * j - 227 < j, written by an earlier batch (B <= 227), and word j + 1 is not yet written.  Returns where it stopped. */
template <int B>
__device__ __forceinline__ int twist_batches(uint32_t *col, size_t pitch, int i, int hi, int off) {
  for (; i + B <= hi; i += B) {
    uint32_t cur[B + 1], far[B];
#pragma unroll
    for (int j = 0; j <= B; j++) cur[j] = col[(size_t)(i + j) * pitch];
#pragma unroll
    for (int j = 0; j < B; j++) far[j] = col[(size_t)(i + j + off) * pitch];
#pragma unroll
    for (int j = 0; j < B; j++) col[(size_t)(i + j) * pitch] = twist_word(cur[j], cur[j + 1], far[j]);
  }
  return i;
}

/* mt19937_gen: one generation in place, in numpy's three ranges.  A lane waits for its loads once per batch: batches of 16, then
 * 4, then 1 make it 45 waits per generation (batches of 32: 26 waits, twice the registers, no faster at 65 536 plants). */
__device__ void twist(uint32_t *col, size_t pitch) {
  int i = twist_batches<16>(col, pitch, 0, MT_N - MT_M, MT_M);
  i = twist_batches<4>(col, pitch, i, MT_N - MT_M, MT_M);
  twist_batches<1>(col, pitch, i, MT_N - MT_M, MT_M);
  i = twist_batches<16>(col, pitch, MT_N - MT_M, MT_N - 1, MT_M - MT_N);
  i = twist_batches<4>(col, pitch, i, MT_N - 1, MT_M - MT_N);
  twist_batches<1>(col, pitch, i, MT_N - 1, MT_M - MT_N);
  col[(size_t)(MT_N - 1) * pitch] = twist_word(col[(size_t)(MT_N - 1) * pitch], col[0], col[(size_t)(MT_M - 1) * pitch]);
}

/* init_genrand: lane p's generator becomes RandomState(s) -- pos = 624 (the first draw twists), no cached gauss */
__device__ __forceinline__ void seed_lane(const npb_noise_t &g, int p, uint32_t s) {
  uint32_t *col = g.key + p;
  col[0] = s;
  for (int i = 1; i < MT_N; i++) {
    s = 1812433253u * (s ^ (s >> 30)) + (uint32_t)i;
    col[(size_t)i * g.pitch] = s;
  }
  g.pos[p] = MT_N;
  g.has_gauss[p] = 0;
  g.gauss[p] = 0.0;
}

__global__ __launch_bounds__(256) void npb_noise_seed_kernel(npb_noise_t g, int n_plants) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_plants) return;
  seed_lane(g, p, ((const uint32_t *)g.pos)[p]);
}

/* k draws of lane p into o[t * n], t = 0 .. k - 1: the lane draws until it has k or its generation is spent; then the wave twists
 * every lane that is out of words, and they go on.  Within a generation a lane loads GROUP words at once and makes up to GROUP / 4
 * polar attempts from them, consuming (pos += 4) only the attempts it makes: one wait for memory per GROUP words instead of per four.
 * Near the end of a generation the words of one attempt are kept in w0..w3 (w0 the oldest), so an attempt whose words straddle a
 * twist resumes after it.
 * k may differ from lane to lane.  Every lane of the wave calls this, and none leaves before the vote finds no lane in need: a lane
 * with k = 0 (one beyond the batch too) touches no memory, never twists and only votes; a lane that has its k draws consumes no
 * further word, so each generator stays numpy's after exactly the calls its lane made.  The vote ends: a lane in need twists, and a
 * fresh generation always yields words. */
constexpr int GROUP = 16;

__device__ __forceinline__ void draw_lane(const npb_noise_t &g, int p, int k, double *o, size_t n) {
  const size_t pitch = g.pitch;
  uint32_t *col = g.key + p;
  int pos = 0, t = 0;
  if (k > 0) {
    pos = g.pos[p];
    if (g.has_gauss[p]) o[(size_t)t++ * n] = g.gauss[p];
  }
  int has = 0;
  double cached = 0.0;
  /* legacy_gauss's loop body on four words: on acceptance f * x2 is drawn and f * x1 cached -- here drawn too if k allows */
  auto attempt = [&](uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    const double x1 = 2.0 * to_double(a, b) - 1.0;
    const double x2 = 2.0 * to_double(c, d) - 1.0;
    const double r2 = x1 * x1 + x2 * x2;
    if (r2 >= 1.0 || r2 == 0.0) return;
    const double f = sqrt(-2.0 * log(r2) / r2);
    o[(size_t)t++ * n] = f * x2;
    if (t < k) o[(size_t)t++ * n] = f * x1;
    else { has = 1; cached = f * x1; }
  };
  uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
  int cnt = 0;
  for (;;) {
    while (t < k) {
      if (cnt == 0 && pos <= MT_N - GROUP) {
        uint32_t w[GROUP];
#pragma unroll
        for (int j = 0; j < GROUP; j++) w[j] = temper(col[(size_t)(pos + j) * pitch]);
#pragma unroll
        for (int j = 0; j < GROUP; j += 4)
          if (t < k) { pos += 4; attempt(w[j], w[j + 1], w[j + 2], w[j + 3]); }
        continue;
      }
      while (cnt < 4 && pos < MT_N) {
        w0 = w1; w1 = w2; w2 = w3;
        w3 = temper(col[(size_t)pos++ * pitch]);
        cnt++;
      }
      if (cnt < 4) break;         /* out of words: twisted below */
      cnt = 0;
      attempt(w0, w1, w2, w3);
    }
    const bool need = t < k;
    if (!__any(need)) break;
    if (need) {
      twist(col, pitch);
      pos = 0;
    }
  }
  if (k > 0) {
    g.pos[p] = pos;
    g.has_gauss[p] = has;
    g.gauss[p] = cached;
  }
}

/* the same k >= 1 for every plant, into out[t * n + p] */
__global__ __launch_bounds__(64) void npb_noise_fill_kernel(npb_noise_t g, int n_plants, int k, double *__restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  draw_lane(g, p, p < n_plants ? k : 0, out + p, (size_t)n_plants);
}

/* ---- the data-gen runner's power profile (maintenance_scenario_runner.py:586-671; nuclear_sim_amd/scenarios.py power_profile_rows
 * is the readable statement).  One lane per plant walks the block's rows; every operation is the reference's, in its order, under
 * this file's flags (no contraction, IEEE division), so the rows are exactly what numpy makes of the same draws. */

/* np.clip(x, 20.0, 105.0) */
__device__ __forceinline__ double profile_raw(double base, double scale, double z) { return fmin(fmax(base + scale * z, 20.0), 105.0); }

/* _apply_power_rate_limit's and _set_target_power's step: wanted if it is within rate of previous, else previous -/+ rate */
__device__ __forceinline__ double limited(double previous, double wanted, double rate) {
  const double change = wanted - previous;
  if (fabs(change) > rate) return change > 0 ? previous + rate : previous - rate;
  return wanted;
}

/* draws row i of a profile of T rows takes from the block: the moving average (T >= 3) looks one draw ahead, so row 0 takes its own
 * draw and row 1's, rows 1 .. T - 2 take the next row's, and the last row none; without it (T < 3) every row takes its own */
__host__ __device__ __forceinline__ int profile_row_draws(int T, int i) { return T < 3 ? 1 : i == 0 ? 2 : i < T - 1 ? 1 : 0; }

/* k rows of one lane from row i of its profile of T rows (0 <= i < T): s = the lane's side column (pitch apart), d = its next
 * draw, the outputs its first row; draws and rows are n apart.  Reads and writes the carried values; returns the row that follows */
__device__ __forceinline__ int rows_lane(int k, int T, int i, double *s, size_t pitch, const double *d, size_t n, double *setpoint_out,
                                         double *target_out, double *z_out) {
  const double base = s[NPB_PROFILE_BASE * pitch], scale = s[NPB_PROFILE_SCALE * pitch];
  double raw_prev = s[NPB_PROFILE_RAW_PREV * pitch], raw = s[NPB_PROFILE_RAW * pitch], z = s[NPB_PROFILE_Z * pitch];
  double target = s[NPB_PROFILE_TARGET * pitch], setpoint = s[NPB_PROFILE_SETPOINT * pitch];
  for (int t = 0; t < k; t++) {
    double sm = raw;                 /* the smoothed value of row i; z: the draw behind its raw value */
    if (T < 3 || i == 0) {
      z = *d; d += n;
      raw = profile_raw(base, scale, z);
      sm = raw;
    }
    if (T >= 3) {
      const double z_row = z;
      if (i < T - 1) {               /* the look-ahead: raw[i + 1] */
        z = *d; d += n;
        const double ahead = profile_raw(base, scale, z);
        if (i > 0) sm = (raw_prev + raw + ahead) / 3.0;
        raw_prev = raw; raw = ahead;
      } else {
        sm = raw;                    /* the last row is left unsmoothed and draws nothing */
      }
      if (z_out) z_out[(size_t)t * n] = z_row;
    } else if (z_out) {
      z_out[(size_t)t * n] = z;
    }
    target = i == 0 ? sm : limited(target, sm, 0.05);
    setpoint = i == 0 ? target : limited(setpoint, target, 0.02);    /* a new profile's ramp starts on its first target */
    if (target_out) target_out[(size_t)t * n] = target;
    setpoint_out[(size_t)t * n] = setpoint;
    if (++i == T) i = 0;
  }
  s[NPB_PROFILE_RAW_PREV * pitch] = raw_prev; s[NPB_PROFILE_RAW * pitch] = raw; s[NPB_PROFILE_Z * pitch] = z;
  s[NPB_PROFILE_TARGET * pitch] = target; s[NPB_PROFILE_SETPOINT * pitch] = setpoint;
  return i;
}

/* draws that k rows from row i of a profile of T rows take: what rows_lane reads, counted the same way */
__host__ __device__ __forceinline__ int profile_draws(int T, int i, int k) {
  int draws = 0;
  for (int t = 0; t < k; t++) {
    draws += profile_row_draws(T, i);
    if (++i == T) i = 0;
  }
  return draws;
}

template <bool RAMP_ONLY>
__global__ __launch_bounds__(256) void npb_profile_rows_kernel(int n_plants, int k, int T, int pos, double *side, size_t pitch,
                                                               const double *draws, const double *target_in, double *setpoint_out,
                                                               double *target_out, double *z_out, double *ramp_prev) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_plants) return;
  const size_t n = (size_t)n_plants;
  if (RAMP_ONLY) {
    double sp = ramp_prev[p];
    for (int t = 0; t < k; t++) {
      const double target = target_in[(size_t)t * n + p];
      sp = isnan(sp) ? target : limited(sp, target, 0.02);
      setpoint_out[(size_t)t * n + p] = sp;
    }
    ramp_prev[p] = sp;
    return;
  }
  rows_lane(k, T, pos, side + p, pitch, draws + p, n, setpoint_out + p, target_out ? target_out + p : nullptr, z_out ? z_out + p : nullptr);
}

/* ---- episode streams (include/npb.h npb_set_episode_streams): the handle's own [block][n] rows of both streams, every plant at a
 * position of its own.  One kernel, one wave per 64 plants, makes rows [from, block) of the blocks for the lanes it works for:
 *   RESTART false: every plant -- the refill of a block that has run out (from = 0; from = block leaves that stream alone);
 *   RESTART true: the plants whose episode index moved since the kernel last looked (restart_all: every plant).  Such a lane gets both
 *     generators seeded anew -- from the bank tables' entry `start[p]` where the restart took a bank entry and the table exists, else
 *     from the plant's own seed --, its profile position, rows made and carried values zeroed, and the rows still pending in the
 *     blocks, [from, block), made again from the new streams' beginning.  A wave without such a lane leaves after one vote.  Behind
 *     a step the same launch first copies the rows the step took into the caller's output columns (`take`): no launch of its own.
 * A lane draws exactly what its rows take: `block - from` draws of the noise, profile_draws(...) of the profile from its own position
 * (one less than the rows where a profile ends in them, one more where one begins: the look-ahead), so each generator stays numpy's
 * after the documented number of calls per plant.  Lanes the kernel does not work for go through draw_lane with k = 0. */
template <bool RESTART>
__global__ __launch_bounds__(64) void npb_episode_streams_kernel(npb_episode_streams_t S, int noise_from, int prof_from, const int32_t *start, int restart_all,
                                                                 npb_episode_streams_take_t take) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n = (size_t)S.n_plants;
  bool work = p < S.n_plants;
  if (RESTART) {
    if (work) {      /* behind a step: the rows it took, into the caller's columns (a restart rewrites only rows no step has taken) */
      if (take.noise_out) take.noise_out[p] = take.noise[p];
      if (take.setpoint_out) take.setpoint_out[p] = take.setpoint[p];
      if (take.target_out) take.target_out[p] = take.target[p];
    }
    work = work && (restart_all || S.episode_index[p] != S.seen_index[p]);
    if (!__any(work)) return;
    if (work) {
      S.seen_index[p] = S.episode_index[p];
      const int32_t s = start ? start[p] : -1;
      const bool entry = s >= 0 && s < S.bank_entries;
      if (S.noise.key) seed_lane(S.noise, p, entry && S.bank_noise_seed ? S.bank_noise_seed[s] : S.own_noise_seed[p]);
      if (S.prof.key) {
        seed_lane(S.prof, p, entry && S.bank_profile_seed ? S.bank_profile_seed[s] : S.own_profile_seed[p]);
        S.position[p] = 0; S.rows_made[p] = 0;
        for (int c = NPB_PROFILE_CARRIED; c < NPB_PROFILE_SIDE; c++) S.prof_side[(size_t)c * S.pitch + p] = 0.0;
      }
    }
  }
  if (S.noise.key && noise_from < S.block)
    draw_lane(S.noise, p, work ? S.block - noise_from : 0, S.noise_rows + (size_t)noise_from * n + p, n);
  if (S.prof.key && prof_from < S.block) {
    const int k = S.block - prof_from, i = work ? S.position[p] : 0;
    draw_lane(S.prof, p, work ? profile_draws(S.steps, i, k) : 0, S.draws + p, n);
    if (work) {
      const size_t row = (size_t)prof_from * n + p;
      S.position[p] = rows_lane(k, S.steps, i, S.prof_side + p, S.pitch, S.draws + p, n, S.setpoint_rows + row, S.target_rows + row, nullptr);
      S.rows_made[p] += k;
    }
  }
}

__global__ __launch_bounds__(256) void npb_profile_set_kernel(double *x, size_t count, double v) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) x[i] = v;
}

}  // namespace

extern "C" {

int npb_profile_draws(int steps, int pos, int k) { return profile_draws(steps, pos, k); }

void npb_launch_profile_rows(int n_plants, int k, int steps, int pos, double *side, size_t pitch, const double *draws,
                             double *setpoint_out, double *target_out, double *z_out, hipStream_t stream) {
  hipLaunchKernelGGL(npb_profile_rows_kernel<false>, dim3((n_plants + 255) / 256), dim3(256), 0, stream, n_plants, k, steps, pos, side, pitch,
                     draws, (const double *)nullptr, setpoint_out, target_out, z_out, (double *)nullptr);
}

void npb_launch_profile_ramp(int n_plants, int k, const double *target_in, double *setpoint_out, double *prev, hipStream_t stream) {
  hipLaunchKernelGGL(npb_profile_rows_kernel<true>, dim3((n_plants + 255) / 256), dim3(256), 0, stream, n_plants, k, 1, 0, (double *)nullptr, (size_t)0,
                     (const double *)nullptr, target_in, setpoint_out, (double *)nullptr, (double *)nullptr, prev);
}

void npb_launch_profile_set(double *x, size_t count, double v, hipStream_t stream) {
  if (count) hipLaunchKernelGGL(npb_profile_set_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, x, count, v);
}

void npb_launch_episode_streams_fill(const npb_episode_streams_t *S, int noise_from, int prof_from, hipStream_t stream) {
  hipLaunchKernelGGL(npb_episode_streams_kernel<false>, dim3((S->n_plants + 63) / 64), dim3(64), 0, stream, *S, noise_from, prof_from, (const int32_t *)nullptr, 0,
                     npb_episode_streams_take_t{});
}

void npb_launch_episode_streams_restart(const npb_episode_streams_t *S, int noise_from, int prof_from, const int32_t *start, int all,
                                        const npb_episode_streams_take_t *take, hipStream_t stream) {
  hipLaunchKernelGGL(npb_episode_streams_kernel<true>, dim3((S->n_plants + 63) / 64), dim3(64), 0, stream, *S, noise_from, prof_from, start, all,
                     take ? *take : npb_episode_streams_take_t{});
}

size_t npb_noise_bytes(size_t pitch) { return pitch * ((size_t)MT_N * sizeof(uint32_t) + 2 * sizeof(int32_t) + sizeof(double)); }

npb_noise_t npb_noise_layout(void *base, size_t pitch) {
  npb_noise_t g;
  char *b = (char *)base;
  g.pitch = pitch;
  g.key = (uint32_t *)b;               b += pitch * MT_N * sizeof(uint32_t);
  g.gauss = (double *)b;               b += pitch * sizeof(double);
  g.pos = (int32_t *)b;                b += pitch * sizeof(int32_t);
  g.has_gauss = (int32_t *)b;
  return g;
}

void npb_launch_noise_seed(npb_noise_t g, int n_plants, hipStream_t stream) {
  hipLaunchKernelGGL(npb_noise_seed_kernel, dim3((n_plants + 255) / 256), dim3(256), 0, stream, g, n_plants);
}

void npb_launch_noise_fill(npb_noise_t g, int n_plants, int k, double *out, hipStream_t stream) {
  hipLaunchKernelGGL(npb_noise_fill_kernel, dim3((n_plants + 63) / 64), dim3(64), 0, stream, g, n_plants, k, out);
}

}  /* extern "C" */
