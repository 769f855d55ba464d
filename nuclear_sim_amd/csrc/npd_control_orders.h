/* npd_control_orders.h -- order rules on the controls' axes (npb_set_control_orders, include/npb.h): 1 to 8 rules, rule r reading the held
 * value of a VALUE axis and ordering one service of one family -- a feedwater pump's (npb_perform_maintenance), a steam generator's, the
 * generator system's, the condenser's or an ejector's (npb_perform_component_maintenance), the turbine's, a bearing's, the lubrication's
 * or a stage's (npb_perform_turbine_maintenance) -- on the plants where it is above the rule's threshold, behind the controls kernel and
 * in front of the step.  nuclear_sim_amd/controls.py (Orders) states which plants fire; what a firing plant gets is what the family's
 * operator kernel (npb_kernels.hip) gives it, through the same section movers and the same handlers, so the bits are theirs.
 *
 * One wave per 64 plants.  The rules are kernel arguments: family, action, unit and option are uniform over the launch, so every
 * dispatch branch is taken by the whole wave -- simpler than the operator kernels, where each lane brings its own action.  At set time
 * the check has refused every rule that cannot succeed on the handle, so here `fire` means success.
 * First pass: latch and restart from the controls' age word as their kernel left it (age == 1: the plant was found unprimed; (age - 1) %
 * interval == 0: its row was read), then per rule one read of held and one of since, `fire`, one write of since and one of fired, all
 * [..][n_plants]: consecutive lanes on consecutive plants.  A wave none of whose lanes fires any rule leaves before NPD_SEGMENT and
 * touches nothing of the arena.  Second pass, r ascending: a rule nobody in the wave fires is skipped; else only the firing lanes load,
 * change and store the sections its action touches (WHICH: npd_order_apply below, the one statement of it in this unit), rule r + 1
 * reading what rule r stored.  A plant on which nothing fires has nothing stored to it.  With a maintenance log each firing is one
 * NPB_MAINT_EVENT_OPERATOR* record (npd_maint_log_operator), stamped with the plant's clock.
 * No LDS, no scratch, no atomics beyond the log's slot hand-out.  Part of npb_attachments.hip, compiled for either storage type. */
#ifndef NPD_CONTROL_ORDERS_H
#define NPD_CONTROL_ORDERS_H

/* one rule on the firing lanes of a wave: the sections the order touches, loaded, handled and stored as the family's operator kernel does.
 * R is uniform over the wave; f64 / N: the arena and its pitch AFTER NPD_SEGMENT */
__device__ __forceinline__ void npd_order_apply(const npb_control_order_t &R, bool fire, npd_real_t *f64, size_t N, size_t p) {
  const int action = R.action, unit = R.unit, option = R.option;
  if (R.family == NPB_ORDER_PUMP) {           /* the ordered pump's section; the handlers read one parameter, the top-off target */
    if (fire) {
      npb_pump_t pm;
      NPD_LOAD(PUMP, npb_pump_t, pm, unit);
      npb_params_t P = {};
      P.maint_top_off_target = R.amount;
      npd_maint_execute(&pm, &P, action, option);
      NPD_STORE(PUMP, npb_pump_t, pm, unit);
    }
  } else if (R.family == NPB_ORDER_COMPONENT) {
    const int kind = npd_component_kind(action);
    if (kind == NPB_COMPONENT_SG) {           /* one generator */
      if (fire) {
        npb_sg_t g;
        NPD_LOAD(SG, npb_sg_t, g, unit);
        npd_sg_maintenance(&g, action, option);
        NPD_STORE(SG, npb_sg_t, g, unit);
      }
    } else if (kind == NPB_COMPONENT_SGSYS && npd_sgsys_touches_generators(action)) {      /* the three generators one after the other */
      int cleaned = 0;
#pragma unroll 1
      for (int k = 0; k < NPB_NUM_SG; k++) {
        if (fire) {
          npb_sg_t g;
          NPD_LOAD(SG, npb_sg_t, g, k);
          npd_sgsys_maintenance_sg(&g, action, &cleaned);
          NPD_STORE(SG, npb_sg_t, g, k);
        }
      }
    } else if (kind == NPB_COMPONENT_SGSYS) {      /* the system's flags alone */
      if (fire) {
        npb_sec_t sec;
        NPD_LOAD(SEC, npb_sec_t, sec, 0);
        npd_sgsys_maintenance_sec(&sec, action);
        NPD_STORE(SEC, npb_sec_t, sec, 0);
      }
    } else if (fire) {                        /* the condenser, with its chemistry for the water treatment; an ejector */
      npb_cond_t cd;
      NPD_LOAD(COND, npb_cond_t, cd, 0);
      if (kind == NPB_COMPONENT_EJECTOR) {
#pragma unroll
        for (int e = 0; e < NPB_NUM_EJECTORS; e++)      /* a constant index: the section stays in registers */
          if (unit == e) npd_ejector_maintenance(&cd, e, action, option);
      } else if (npd_cond_touches_chemistry(action)) {
        npb_chem_t ch;      /* chem[1]: the condenser-owned WaterChemistry (include/npb_fields.h) */
        NPD_LOAD(CHEM, npb_chem_t, ch, 1);
        npd_cond_maintenance(&cd, &ch, action, option);
        NPD_STORE(CHEM, npb_chem_t, ch, 1);
      } else {
        npd_cond_maintenance(&cd, nullptr, action, option);
      }
      NPD_STORE(COND, npb_cond_t, cd, 0);
    }
  } else {
    const int kind = npd_turbine_kind(action);
    if (kind != NPB_TURBINE_STAGE) {          /* the turb section: the turbine, a bearing, the lubrication system */
      if (fire) {
        npb_turb_t t;
        NPD_LOAD(TURB, npb_turb_t, t, 0);
        if (kind == NPB_TURBINE_SYSTEM) npd_turbine_system_maintenance(&t, action);
        else if (kind == NPB_TURBINE_LUBE) npd_turbine_lube_maintenance(&t, action);
        else {
#pragma unroll
          for (int b = 0; b < 4; b++)      /* a constant index: the section stays in registers */
            if (unit == b) npd_turbine_bearing_maintenance(&t, b, action);
        }
        NPD_STORE(TURB, npb_turb_t, t, 0);
      }
    } else if (fire) {                        /* the ordered stage's three tstg columns and nothing else (carried reals: slot = column) */
      npd_real_t *deg = (npd_real_t *)npd_gaddr(f64, N, p, NPD_SEC_COL(TSTG, 0) + NPB_F64_SLOT(npb_tstg_t, stage_efficiency_degradation) + unit);
      npd_real_t *dep = (npd_real_t *)npd_gaddr(f64, N, p, NPD_SEC_COL(TSTG, 0) + NPB_F64_SLOT(npb_tstg_t, stage_deposit_thickness) + unit);
      npd_real_t *wear = (npd_real_t *)npd_gaddr(f64, N, p, NPD_SEC_COL(TSTG, 0) + NPB_F64_SLOT(npb_tstg_t, stage_blade_wear_factor) + unit);
      double efficiency_degradation = (double)*deg, deposit_thickness = (double)*dep, blade_wear_factor = (double)*wear;
      npd_turbine_stage_maintenance(&efficiency_degradation, &deposit_thickness, &blade_wear_factor, action);
      *deg = (npd_real_t)efficiency_degradation; *dep = (npd_real_t)deposit_thickness; *wear = (npd_real_t)blade_wear_factor;
    }
  }
}
/* the record kind of a family, and the bearing byte of its record (a pump's bearing replacement names its bearing; else 0) */
__device__ __forceinline__ int npd_order_event_kind(int family) {
  return family == NPB_ORDER_PUMP ? NPB_MAINT_EVENT_OPERATOR : family == NPB_ORDER_COMPONENT ? NPB_MAINT_EVENT_OPERATOR_COMPONENT : NPB_MAINT_EVENT_OPERATOR_TURBINE;
}

__global__ __launch_bounds__(NPB_WAVE) void npb_control_orders_kernel(npd_real_t *__restrict__ f64, size_t N, npb_control_orders_t O, npd_maint_log_t L, int n_plants) {
  const size_t block_base = (size_t)blockIdx.x * NPB_WAVE;
  const size_t p = block_base + threadIdx.x, n = (size_t)n_plants;
  const bool live = p < n;
  /* 1. who fires what: the statement's recurrence on since, fired written for every live plant */
  uint32_t fires = 0;
  if (live) {
    const int32_t age = O.age[p];             /* as the controls kernel left it on this step: >= 1 */
    const bool restart = age == 1, latch = (age - 1) % O.interval == 0;
#pragma unroll 1
    for (int r = 0; r < O.n_orders; r++) {
      const npb_control_order_t &R = O.rule[r];
      const size_t cell = (size_t)r * n + p;
      const int32_t c = restart ? NPB_CONTROL_ORDER_NEVER : O.since[cell];
      const double y = O.held[(size_t)R.axis * n + p];
      const bool fire = latch && y > R.threshold && (c == NPB_CONTROL_ORDER_NEVER || c >= R.min_interval);
      O.since[cell] = fire ? 1 : (c >= NPB_CONTROL_ORDER_NEVER - 1 ? c : c + 1);
      O.fired[cell] = fire ? 1.0 : 0.0;
      fires |= (uint32_t)fire << r;
    }
  }
  if (!__any(fires != 0)) return;
  /* 2. the service, rule by rule */
  NPD_SEGMENT(f64, N, block_base);
#pragma unroll 1
  for (int r = 0; r < O.n_orders; r++) {
    const bool fire = ((fires >> r) & 1u) != 0;
    if (!__any(fire)) continue;
    const npb_control_order_t &R = O.rule[r];
    npd_order_apply(R, fire, f64, N, p);
    if (L.cursor) {
      double t = 0.0;
      if (fire) t = NPD_F64_COL(PRIM, npb_prim_t, sim_time, 0);
      npd_maint_log_operator(L, fire, p, t, R.unit, R.action, npd_order_event_kind(R.family),
                             R.family == NPB_ORDER_PUMP && R.action == NPB_MA_BEARING_REPLACEMENT ? R.option : 0);
    }
  }
}
static void NPB_LAUNCHER(control_orders)(void *arena, size_t npad, const npb_control_orders_t *O, npd_maint_log_t log, int n_plants, hipStream_t stream) {
  hipLaunchKernelGGL(npb_control_orders_kernel, dim3((unsigned)((n_plants + NPB_WAVE - 1) / NPB_WAVE)), dim3(NPB_WAVE), 0, stream, (npd_real_t *)arena,
                     npad, *O, log, n_plants);
}
#endif
