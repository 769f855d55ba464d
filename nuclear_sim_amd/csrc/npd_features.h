/* npd_features.h -- the caller's policy inputs (npb_set_features, include/npb.h): up to 64 columns, each through a transform, as a
 * contiguous [n_plants][K][C] tensor of the last K frames (k = K - 1 the newest), float or double, kept on the device behind every step.
 * nuclear_sim_amd/features.py states it in numpy; this file produces its bits: the subtraction is rounded before the product
 * (-ffp-contract=off), the NaN replacement comes before the clip, the clip is two comparisons that a NaN passes, the narrowing is the
 * hardware's round-to-nearest-even with subnormals kept.
 *
 * ONE kernel, three modes.  NPD_FEATURES_STEP (pass A, behind every step): every plant's frame of this step, all columns live; a primed
 * plant of the episode last seen shifts its stack by one frame and appends, any other has all K slots filled.  NPD_FEATURES_RESTART (pass
 * B, behind the episode kernel): a plant whose carried episode index differs from the one seen was restarted on this step -- its stack,
 * terminal frame included, goes to final[p] where the caller keeps one, then all K slots take the FRESH frame of the restored state
 * (members and sources marked live are read, every other side column is its `fresh` constant).  NPD_FEATURES_PRIME: the unprimed plants'
 * slots take the fresh frame.  A wave of pass B or of the priming none of whose lanes is concerned ends after its bookkeeping loads.
 *
 * One wave per 64 plants.  Column reads have consecutive lanes on consecutive plants (npd_column_read), the segmented arena goes through
 * NPD_SEGMENT, the descriptors are uniform over the launch: scalar loads.  A lane asks for its columns sixteen at a time, each column and
 * its second column before the first transform of the sixteen, and nothing is stored to memory before the last column load: the frame
 * goes to LDS, row = plant, with an odd row stride (C | 1) so that the 64 lanes of a column store hit 64 banks -- 64 x 65 elements, 16.25
 * KiB for float and 32.5 KiB for double.
 * Neither the frame store nor the shift is one lane per plant row (K x C elements between lanes): the 64 plants of a wave own ONE
 * contiguous block of 64 x K x C elements of `out`, and the wave walks it with consecutive lanes on consecutive elements, W elements per
 * lane (16 bytes where C and the buffer's alignment allow, else one element).  Element e takes either its successor by C (the shift) or
 * the LDS frame (the newest slot, or every slot of a filling plant).  The walk is IN PLACE and ascending, in groups of eight chunks of 64
 * x W elements: a group's loads are all issued (eight in flight per lane), then the group's stores, in chunk order.  This is safe:
 * element e is read by element e - C only, which lies in the same or an earlier chunk, so its load stands before the store in program
 * order (the barrier between a group's loads and its stores keeps the compiler to that); a chunk's store carries the data of that
 * chunk's load, so it issues only when that load has returned, and loads return in order: every load of the same or an earlier chunk
 * has returned by then.  The loads still in flight, of later chunks, touch only elements above the chunk being stored.  The copy to `final` and the refill of pass B and of the priming go per concerned plant, all 64 lanes on its K x C contiguous
 * elements, as the event windows copy a captured lane's window.
 * No scratch, no atomics.  Part of npb_attachments.hip, compiled for either storage type: it reads
 * the arena.
 * NOT here (include/npb.h says so too): the terminal stack in the episode records, half-precision output, a delta or rate kind (the
 * stack carries it).  Running statistics updated on the device are the normaliser's (npd_normalizer.h): it rewrites `ref` and `scale`
 * of the table this kernel reads, in front of pass A. */
#ifndef NPD_FEATURES_H
#define NPD_FEATURES_H

enum { NPD_FEATURES_STEP = 0, NPD_FEATURES_RESTART = 1, NPD_FEATURES_PRIME = 2 };
#define NPD_FEATURES_CHUNK 16      /* columns asked for together: 2 x 16 doubles in registers */
#define NPD_FEATURES_GROUP 8       /* chunks of the walk whose loads are in flight together */
#define NPD_FEATURES_ROW (NPB_FEATURES_COLS_MAX + 1)

/* one column's value from its raw sample(s): the statement's transform, in its order */
__device__ __forceinline__ double npd_feature_transform(const npb_feature_col_t &D, double v, double ref) {
  double y;
  if (D.kind == NPB_FEATURE_KIND_BITS) y = ((uint32_t)(int32_t)v & D.mask) != 0u ? 1.0 : 0.0;
  else { const double d = v - ref; y = d * D.scale; }
  if (y != y) y = D.nan_to;      /* (a NaN nan_to arrives as THE quiet NaN: the bits of a NaN that stays are fixed) */
  y = y < D.lo ? D.lo : y;
  y = y > D.hi ? D.hi : y;
  return y;
}

template <typename OUT, int W>
__global__ __launch_bounds__(NPB_WAVE) void npb_features_kernel(const npd_real_t *__restrict__ f64, size_t N, npb_features_t F, int n_plants, int mode,
                                                                const int32_t *__restrict__ index) {
  typedef npd_features_vec<OUT, W> V;
  __shared__ OUT frame[NPB_WAVE * NPD_FEATURES_ROW];
  const size_t block_base = (size_t)blockIdx.x * NPB_WAVE;
  NPD_SEGMENT(f64, N, block_base);
  const int lane = threadIdx.x;
  const size_t p = block_base + lane, n = (size_t)n_plants;
  const int C = F.n_cols, K = F.stack, KC = K * C, Cs = C | 1;
  /* 1. the bookkeeping words: who fills (pass A), who restarted (pass B), who is unprimed (priming) */
  bool concerned = false, fill = false;
  int32_t episode = 0;
  if (p < n) {
    const int32_t primed = F.primed[p], seen = F.seen[p];
    episode = index ? index[p] : seen;
    if (mode == NPD_FEATURES_STEP) { concerned = true; fill = !primed || episode != seen; }
    else if (mode == NPD_FEATURES_RESTART) concerned = episode != seen;
    else concerned = !primed;
  }
  const uint64_t rows = __ballot(concerned), filling = __ballot(fill);
  if (!rows) return;
  /* 2. the frame into LDS: live in pass A; fresh otherwise -- members and live sources read, the other side columns their constants */
  const bool live = mode == NPD_FEATURES_STEP;
  if (concerned) {
    for (int c0 = 0; c0 < C; c0 += NPD_FEATURES_CHUNK) {
      double v[NPD_FEATURES_CHUNK], ref[NPD_FEATURES_CHUNK];
#pragma unroll
      for (int j = 0; j < NPD_FEATURES_CHUNK; j++) {
        v[j] = ref[j] = 0.0;
        if (c0 + j < C) {
          const npb_feature_col_t &D = F.cols[c0 + j];
          v[j] = live || (D.live & 1) ? npd_column_read<const npb_colstat_col_t &>(f64, N, p, D.c) : D.fresh;
          ref[j] = !D.ref_col ? D.ref : live || (D.live & 2) ? npd_column_read<const npb_colstat_col_t &>(f64, N, p, D.r) : D.ref;
        }
      }
#pragma unroll
      for (int j = 0; j < NPD_FEATURES_CHUNK; j++)
        if (c0 + j < C) frame[lane * Cs + c0 + j] = (OUT)npd_feature_transform(F.cols[c0 + j], v[j], ref[j]);
    }
    F.primed[p] = 1;
    F.seen[p] = episode;
  }
  __syncthreads();
  const int in_block = n - block_base < (size_t)NPB_WAVE ? (int)(n - block_base) : NPB_WAVE;
  OUT *block = (OUT *)F.out + block_base * (size_t)KC;
  if (mode == NPD_FEATURES_STEP) {
    /* 3a. the walk over the wave's block, in place and ascending (the header says why that is safe) */
    /* plant and slot of an element by a float multiply: e + 0.5 is exact below 2^24, the true quotient's fraction lies at least 1 / 512 (of
     * the second division: 1 / 128) from an integer, and the product is off by less than 2^-13: the truncation is the integer quotient */
    const int total = in_block * KC;
    const float per_kc = 1.0f / (float)KC, per_c = 1.0f / (float)C;
    for (int e0 = 0; e0 < total; e0 += NPB_WAVE * W * NPD_FEATURES_GROUP) {
      V x[NPD_FEATURES_GROUP];
#pragma unroll
      for (int u = 0; u < NPD_FEATURES_GROUP; u++) {
        const int e = e0 + (u * NPB_WAVE + lane) * W;
        if (e >= total) continue;
        const int r = (int)(((float)e + 0.5f) * per_kc), rem = e - r * KC, k = (int)(((float)rem + 0.5f) * per_c), c = rem - k * C;
        if (((filling >> r) & 1u) || k == K - 1) {
#pragma unroll
          for (int w = 0; w < W; w++) x[u].x[w] = frame[r * Cs + c + w];
        } else {
          x[u] = *(const V *)(block + e + C);
        }
      }
      __syncthreads();      /* the group's loads stand before its stores */
#pragma unroll
      for (int u = 0; u < NPD_FEATURES_GROUP; u++) {
        const int e = e0 + (u * NPB_WAVE + lane) * W;
        if (e < total) *(V *)(block + e) = x[u];
      }
    }
    return;
  }
  /* 3b. pass B and the priming: one concerned plant after the other, all 64 lanes on its K x C elements -- the stack that ended into
   * final[p] first (pass B with a final buffer), then the fresh frame into every slot */
  OUT *final = mode == NPD_FEATURES_RESTART ? (OUT *)F.final : nullptr;
  for (uint64_t left = rows; left; left &= left - 1) {
    const int r = __ffsll((unsigned long long)left) - 1;
    OUT *row = block + (size_t)r * KC;
    for (int i = lane * W; i < KC; i += NPB_WAVE * W) {
      if (final) *(V *)(final + (block_base + (size_t)r) * KC + i) = *(const V *)(row + i);
      const int c = i % C;
      V x;
#pragma unroll
      for (int w = 0; w < W; w++) x.x[w] = frame[r * Cs + c + w];
      *(V *)(row + i) = x;
    }
  }
}
/* W: 16 bytes per lane where every frame is a whole number of them and both buffers are 16-byte aligned, else one element */
static void NPB_LAUNCHER(features)(const void *arena, size_t npad, const npb_features_t *F, int n_plants, int mode, const int32_t *index, hipStream_t stream) {
  const dim3 grid((unsigned)((n_plants + NPB_WAVE - 1) / NPB_WAVE)), block(NPB_WAVE);
  const int per16 = F->out_f64 ? 2 : 4;
  const bool wide = F->n_cols % per16 == 0 && (((uintptr_t)F->out | (uintptr_t)F->final) & 15u) == 0;
#define NPD_FEATURES_LAUNCH(OUT, W) hipLaunchKernelGGL((npb_features_kernel<OUT, W>), grid, block, 0, stream, (const npd_real_t *)arena, npad, *F, n_plants, mode, index)
  if (F->out_f64) { if (wide) NPD_FEATURES_LAUNCH(double, 2); else NPD_FEATURES_LAUNCH(double, 1); }
  else { if (wide) NPD_FEATURES_LAUNCH(float, 4); else NPD_FEATURES_LAUNCH(float, 1); }
#undef NPD_FEATURES_LAUNCH
}
#endif
