/* npb_noise.h -- host-callable launchers of the heat-source noise generator and of the power profile's filter (npb_noise.hip;
 * internal to libnpb.so).
 * One MT19937 stream per plant, numpy's legacy RandomState: key [624][pitch] uint32 (word i of every plant contiguous),
 * pos / has_gauss int32 [pitch], gauss double [pitch]. */
#ifndef NPB_NOISE_H
#define NPB_NOISE_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define NPB_MT_N 624
typedef struct {
  uint32_t *key;       /* [NPB_MT_N][pitch] */
  int32_t *pos;        /* [pitch] */
  int32_t *has_gauss;  /* [pitch] */
  double *gauss;       /* [pitch] */
  size_t pitch;
} npb_noise_t;
/* bytes of one allocation holding the four arrays for `pitch` plants, and the arrays carved out of it */
size_t npb_noise_bytes(size_t pitch);
npb_noise_t npb_noise_layout(void *base, size_t pitch);
/* init_genrand: plant p's seed is read from (uint32_t *)g.pos [p] (the caller puts it there), then pos = 624, no cached gauss */
void npb_launch_noise_seed(npb_noise_t g, int n_plants, hipStream_t stream);
/* the next k standard_normal() draws of every plant into out[t * n_plants + p] */
void npb_launch_noise_fill(npb_noise_t g, int n_plants, int k, double *out, hipStream_t stream);

/* The data-gen runner's power profile (include/npb.h, npb_profile_*): rows from a block of draws of the profile's own generators.
 * Per plant, [NPB_PROFILE_SIDE][pitch] doubles: its load profile (base, and min(0.2, std) already taken) and what the filter carries
 * from one row to the next -- the clipped raw values of the previous row and of this one (this one's is the moving average's one-draw
 * look-ahead of the previous row), the draw behind the latter, the previous target and the previous setpoint. */
enum { NPB_PROFILE_BASE = 0, NPB_PROFILE_SCALE, NPB_PROFILE_CARRIED, /* then the carried values, in npb_profile_get_state's order: */
       NPB_PROFILE_RAW_PREV = NPB_PROFILE_CARRIED, NPB_PROFILE_RAW, NPB_PROFILE_Z, NPB_PROFILE_TARGET, NPB_PROFILE_SETPOINT, NPB_PROFILE_SIDE };
#define NPB_PROFILE_NUM_CARRIED (NPB_PROFILE_SIDE - NPB_PROFILE_CARRIED)
/* draws that rows [pos, pos + k) of profiles of `steps` rows consume (pos: rows already made of the current profile, 0 <= pos < steps):
 * the kernel's own count, so the block it is given is exactly as long as what it reads */
int npb_profile_draws(int steps, int pos, int k);
/* k rows from position pos on: draws [npb_profile_draws(steps, pos, k)][n_plants] in, setpoint_out / target_out / z_out [k][n_plants]
 * out (the last two may be NULL); side is read and its carried rows written */
void npb_launch_profile_rows(int n_plants, int k, int steps, int pos, double *side, size_t pitch, const double *draws,
                             double *setpoint_out, double *target_out, double *z_out, hipStream_t stream);
/* the ramp stage alone: setpoint_out[t] from target_in[t] ([k][n_plants] each; they may be the same block) and the carried previous
 * setpoint prev [n_plants] (NaN = none yet: the first setpoint is the first target), which is updated */
void npb_launch_profile_ramp(int n_plants, int k, const double *target_in, double *setpoint_out, double *prev, hipStream_t stream);
/* v into x[0 .. count) */
void npb_launch_profile_set(double *x, size_t count, double v, hipStream_t stream);

/* Episode streams (include/npb.h npb_set_episode_streams): what the handle owns while the mode is on, as the kernels read it.  A stream
 * the handle has no generators for has key = NULL and its rows NULL. */
typedef struct {
  int n_plants, block, steps;                          /* steps: the profile's horizon */
  size_t pitch;
  npb_noise_t noise, prof;
  double *prof_side;                                   /* [NPB_PROFILE_SIDE][pitch], the profile's own */
  double *noise_rows, *setpoint_rows, *target_rows;    /* [block][n_plants] */
  double *draws;                                       /* [block + 1][n_plants]: the profile's draws on their way to rows */
  int32_t *position, *rows_made;                       /* [pitch]: row of the current profile the next row made is, rows made since the restart */
  const uint32_t *own_noise_seed, *own_profile_seed;   /* [pitch]: as given to npb_noise_seed / npb_profile_seed */
  const uint32_t *bank_noise_seed, *bank_profile_seed; /* [bank_entries] each, or NULL */
  int bank_entries;
  const int32_t *episode_index;                        /* [pitch], the handle's (npb_set_autoreset) */
  int32_t *seen_index;                                 /* [pitch]: its value when the plant's streams last began */
} npb_episode_streams_t;
typedef struct { const double *noise, *setpoint, *target; double *noise_out, *setpoint_out, *target_out; } npb_episode_streams_take_t;
/* rows [noise_from, block) of the noise block and [prof_from, block) of the profile's for every plant, from where its streams are
 * (from = block: that stream is left alone) */
void npb_launch_episode_streams_fill(const npb_episode_streams_t *S, int noise_from, int prof_from, hipStream_t stream);
/* the plants whose episode index is not the one seen (all != 0: every plant): streams seeded anew -- from the bank tables' entry
 * start[p] where start is given, the entry is one and the table exists, else from the plant's own seed --, position, rows made and
 * carried values zeroed, seen = index, and the same rows made from the new streams' beginning.  take (NULL = none): one [n_plants] row
 * each that the launch first copies into the caller's column; a pair with a NULL output is skipped */
void npb_launch_episode_streams_restart(const npb_episode_streams_t *S, int noise_from, int prof_from, const int32_t *start, int all,
                                        const npb_episode_streams_take_t *take, hipStream_t stream);
#ifdef __cplusplus
}
#endif
#endif
