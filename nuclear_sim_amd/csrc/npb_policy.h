/* npb_policy.h -- host-callable launchers of the policy (npb_policy.hip; internal to libnpb.so; include/npb.h and
 * nuclear_sim_amd/policy.py state what they compute). */
#ifndef NPB_POLICY_H
#define NPB_POLICY_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/npb.h"
#ifdef __cplusplus
extern "C" {
#endif
#define NPD_POLICY_LAYERS_MAX (NPB_POLICY_HIDDEN_MAX + 1)      /* the hidden layers and the head */
/* one layer: `in` inputs (in_pad: the next multiple of 4), `out` outputs (out_pad: the next multiple of 32); its bias at theta + b, its
 * weights as the caller packed them at theta + w, and as the kernel reads them at padded + wp: Wt[in_pad][out_pad], the cells beyond `in`
 * and beyond `out` +0.0 */
typedef struct { int in, in_pad, out, out_pad; uint32_t w, b, wp; } npd_policy_layer_t;
typedef struct { int n_layers; npd_policy_layer_t layer[NPD_POLICY_LAYERS_MAX]; } npd_policy_net_t;
/* what the handle keeps of a set policy: the shapes, the caller's descriptor, and ONE device allocation (base theta): theta
 * [theta_count] | padded [padded_count] */
typedef struct {
  float *theta; float *padded;
  uint32_t theta_count, padded_count, log_std, std;      /* (log_std, std: offsets into theta) */
  npd_policy_net_t actor, critic;
  int cells, n_axes, width_max;      /* K * C; A; the widest hidden layer of either net */
  npb_policy_desc_t D;
} npb_policy_t;
/* one launch of the nets over `rows` rows of x ([rows][cells], float or double).  act != NULL: the step's launch -- actor, noise, critic,
 * every output; act == NULL: the critic alone into value (npb_policy_values) */
typedef struct {
  const void *x; int x_f64, rows;
  void *act; int act_f64;
  float *value, *logp, *extras; int n_extras, value_slot, logp_slot;
  uint64_t seed, t; uint32_t first; int deterministic;
} npd_policy_run_t;
/* the shapes of a descriptor laid out: every offset and count of *P but its pointers */
void npb_policy_layout(const npb_policy_desc_t *D, int cells, int n_axes, npb_policy_t *P);
void npb_launch_policy_repack(const npb_policy_t *P, hipStream_t stream);
void npb_launch_policy(const npb_policy_t *P, const npd_policy_run_t *R, hipStream_t stream);
/* the z of draw t ([n][A] double) and, where words != NULL, the Philox words behind it ([n][(A + 1) / 2][4] uint32) */
void npb_launch_policy_noise(const npb_policy_t *P, uint64_t t, int n_plants, double *z, uint32_t *words, hipStream_t stream);
#ifdef __cplusplus
}
#endif
#endif
