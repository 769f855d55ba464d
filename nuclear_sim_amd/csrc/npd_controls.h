/* npd_controls.h -- the caller's policy outputs (npb_set_controls, include/npb.h): 1 to 8 axes, axis a reading element [p][a] of the
 * caller's contiguous [n_plants][n_axes] tensor of float or double, each through a transform and then either a move of one of the four
 * actuator members (RATE, TARGET), a value of one of the step's two input columns (COLUMN) or nothing but the hold (VALUE), in front of
 * every step.
 * nuclear_sim_amd/controls.py states it in numpy; this file produces its bits: the product is rounded before the sum
 * (-ffp-contract=off), the NaN replacement comes before the affine map, the clip is two comparisons, the deadband a strict one.
 *
 * Both actuator kinds go through npd_apply_control_actions (npd_primary.h), the function the step kernels call for step(action,
 * magnitude): the rate expressions and the range limits are stated there and nowhere else.  The four members are read by the step only
 * inside npd_primary_update, behind that call, and in the observation at the end; nothing in front of the primary update reads them, and
 * the maintenance screen's cooldown cache watches the feedwater pumps' parameters, not these four: moving them here and stepping with
 * NO_ACTION is the step with that action.
 *
 * One wave per 64 plants.  The wave's 64 rows of `in` are ONE contiguous run of 64 x n_axes elements: it is loaded with consecutive lanes
 * on consecutive elements (n_axes loads per lane, coalesced for every axis count and element type, an odd n_axes whose rows are not
 * 16-byte aligned included) and transposed through LDS, row = plant, with an odd row stride (n_axes | 1) so that the 64 lanes of an axis
 * read hit 64 banks.  The ragged last wave loads the live rows only; a wave none of whose plants latches on this step (interval > 1)
 * loads nothing.  The axes are uniform over the launch (kernel arguments: scalar loads), so every branch on an axis' kind or target is
 * taken by the whole wave.  held / prev / the input columns are [..][n_plants]: consecutive lanes on consecutive plants.
 * The state goes through NPD_SEGMENT and the per-member addresses the operator-maintenance kernels use, for either storage type and the
 * segmented arena.  A lane stores a member only where the bits it would store differ from the bits it loaded: a plant whose actuators
 * do not move has nothing stored to it; under float storage a moved member is rounded to float at this store (as npb_set_field rounds).
 * No scratch, no atomics.  Part of npb_attachments.hip, compiled for either storage type. */
#ifndef NPD_CONTROLS_H
#define NPD_CONTROLS_H

#define NPD_CONTROLS_ROW (NPB_CONTROLS_AXES_MAX + 1)

/* the statement's transform of one element, in its order */
__device__ __forceinline__ double npd_control_transform(const npb_control_axis_t &D, double x) {
  if (x != x) x = D.nan_to;
  const double scaled = x * D.scale;
  double y = scaled + D.offset;
  y = y < D.lo ? D.lo : y;
  y = y > D.hi ? D.hi : y;
  if (D.kind == NPB_CONTROL_KIND_RATE && fabs(y) < D.deadband) y = 0.0;
  return y;
}

/* what npd_apply_control_actions makes of an actuator at `pos`: its increasing (up) or decreasing ControlAction code at magnitude mag */
__device__ __forceinline__ double npd_control_move(const npb_params_t *P, int actuator, bool up, double pos, double mag) {
  npb_prim_t s;
  s.control_rod_position = s.coolant_flow_rate = s.steam_valve_position = s.boron_concentration = pos;
  switch (actuator) {
    case NPB_ACTUATOR_ROD: npd_apply_control_actions(&s, P, up ? 1 : 0, mag, P->dt); return s.control_rod_position;
    case NPB_ACTUATOR_FLOW: npd_apply_control_actions(&s, P, up ? 2 : 3, mag, P->dt); return s.coolant_flow_rate;
    case NPB_ACTUATOR_VALVE: npd_apply_control_actions(&s, P, up ? 4 : 5, mag, P->dt); return s.steam_valve_position;
    default: npd_apply_control_actions(&s, P, up ? 10 : 9, mag, P->dt); return s.boron_concentration;
  }
}
/* the member slot of an actuator in the primary section (carried reals: slot = column within the section) */
__device__ __forceinline__ int npd_control_slot(int actuator) {
  switch (actuator) {
    case NPB_ACTUATOR_ROD: return NPB_F64_SLOT(npb_prim_t, control_rod_position);
    case NPB_ACTUATOR_FLOW: return NPB_F64_SLOT(npb_prim_t, coolant_flow_rate);
    case NPB_ACTUATOR_VALVE: return NPB_F64_SLOT(npb_prim_t, steam_valve_position);
    default: return NPB_F64_SLOT(npb_prim_t, boron_concentration);
  }
}

template <typename IN>
__global__ __launch_bounds__(NPB_WAVE) void npb_controls_kernel(npd_real_t *__restrict__ f64, size_t N, npb_controls_t C, npb_params_t P, int n_plants,
                                                                const int32_t *__restrict__ index) {
  __shared__ IN rows[NPB_WAVE * NPD_CONTROLS_ROW];
  const size_t block_base = (size_t)blockIdx.x * NPB_WAVE;
  NPD_SEGMENT(f64, N, block_base);
  const int lane = threadIdx.x;
  const size_t p = block_base + lane, n = (size_t)n_plants;
  const int A = C.n_axes, As = A | 1;
  const bool live = p < n;
  /* 1. the bookkeeping words: who starts a new hold, who latches on this step */
  bool primed = false, latch = false;
  int32_t age = 0, episode = 0;
  if (live) {
    const int32_t seen = C.seen[p];
    episode = index ? index[p] : seen;
    primed = C.primed[p] != 0 && episode == seen;
    if (primed) age = C.age[p];
    latch = age % C.interval == 0;
  }
  /* 2. the wave's run of `in` into LDS, transposed: element e of the run is axis e % A of row e / A (e < 64 * 8: the float quotient of
   * e + 0.5 is off by less than 2^-14 and at least 1 / 16 from an integer, so its truncation is the integer quotient) */
  if (__any(latch)) {
    const int in_block = n - block_base < (size_t)NPB_WAVE ? (int)(n - block_base) : NPB_WAVE;
    const int total = in_block * A;
    const IN *run = (const IN *)C.in + block_base * (size_t)A;
    const float per_a = 1.0f / (float)A;
    for (int e = lane; e < total; e += NPB_WAVE) {
      const int r = (int)(((float)e + 0.5f) * per_a), a = e - r * A;
      rows[r * As + a] = run[e];
    }
  }
  __syncthreads();
  if (!live) return;
  /* 3. axis by axis: the value held, then its move or its column */
  for (int a = 0; a < A; a++) {
    const npb_control_axis_t &D = C.axes[a];
    double *held = C.held + (size_t)a * n + p;
    double y;
    if (latch) {
      y = npd_control_transform(D, (double)rows[lane * As + a]);
      C.prev[(size_t)a * n + p] = primed ? *held : y;
      *held = y;
    } else {
      y = *held;
    }
    if (D.kind == NPB_CONTROL_KIND_VALUE) continue;      /* held, for whoever reads the column */
    if (D.kind == NPB_CONTROL_KIND_COLUMN) { C.column[D.target][p] = y; continue; }
    npd_real_t *member = (npd_real_t *)npd_gaddr(f64, N, p, NPD_SEC_COL(PRIM, 0) + npd_control_slot(D.target));
    const double pos = (double)*member;
    double moved = pos;
    if (D.kind == NPB_CONTROL_KIND_RATE) {
      if (y > 0.0) moved = npd_control_move(&P, D.target, true, pos, y);
      else if (y < 0.0) moved = npd_control_move(&P, D.target, false, pos, -y);
    } else {
      if (y > pos) moved = npd_pymin(npd_control_move(&P, D.target, true, pos, D.max_magnitude), y);
      else if (y < pos) moved = npd_pymax(npd_control_move(&P, D.target, false, pos, D.max_magnitude), y);
    }
    if (npd_real_bits(moved) != npd_real_bits(pos)) *member = (npd_real_t)moved;
  }
  C.age[p] = age + 1;
  C.primed[p] = 1;
  C.seen[p] = episode;
}
static void NPB_LAUNCHER(controls)(void *arena, size_t npad, const npb_controls_t *C, const npb_params_t *P, int n_plants, const int32_t *index, hipStream_t stream) {
  const dim3 grid((unsigned)((n_plants + NPB_WAVE - 1) / NPB_WAVE)), block(NPB_WAVE);
  if (C->in_f64) hipLaunchKernelGGL(npb_controls_kernel<double>, grid, block, 0, stream, (npd_real_t *)arena, npad, *C, *P, n_plants, index);
  else hipLaunchKernelGGL(npb_controls_kernel<float>, grid, block, 0, stream, (npd_real_t *)arena, npad, *C, *P, n_plants, index);
}
#endif
