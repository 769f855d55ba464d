"""GPU: the recurrent training kernels (npb_ppo_seq.hip: npb_ppo_seq_kernel for whole sequences and for truncated segments,
npb_segment_starts_kernel for the refresh; npb_policy_core.hip's recording of the stored states) at the shapes, types and places in time
where they have logic of their own and the three suites written with the features (test_recurrent_gpu.py, test_recurrent_train_gpu.py,
test_segments_gpu.py) never went -- against the same numpy statement (nuclear_sim_amd.recurrent), by the same contracts and through the
same helpers: hard gates with relu nets give logp_new, value_new and hidden by bits, the ratio within 4 ulp of numpy's, and grad, stats and
more by bits once the statement is fed the device's ratio; soft gates with tanh nets may stand 8 times as far from float64 autograd as the
statement does.  No tolerance is new here.

THE SHAPE TABLE (``TABLE``).  Both launchers pick the small-LDS build <64, 64> by npd_policy_small(P, H): ``cells <= 64 && width_max <= 64
&& H <= 64``; the seven H-wide LDS buffers are H_MAX x 33 floats, H_MAX covering the core and both nets.

    a  16 x 4 = 64 cells, H 64, (64,) / (64,), 2 axes            everything AT the small build's limit: a rule with ``<`` for ``<=`` sends it
                                                                 to the large build (same bits, so only the table's neighbours show it); an
                                                                 index that runs one past 64 rows in the small build shows here
    b  16 x 4 = 64 cells, H 65, (7,) / (9,), 4 axes              the core alone one past: a rule without its third term runs b1 .. b6[64][row]
                                                                 past the 64-row buffers, h' of unit 64 lands in the next buffer
    c  13 x 5 = 65 cells, H 64, (7,) / (9,), 3 axes              the cells alone one past: xs[64][row] past the small xs
    d  16 x 4 = 64 cells, H 5, (7,) / (65,), 3 axes              one net alone one past, behind a tiny core: H_MAX covers the nets, and a rule
                                                                 that looked at the core and the actor alone puts the critic's 65th unit past b2
    e  25 x 4 = 100 cells, H 127, (100, 96) / (127,), 5 axes     ragged k- and j-blocks of the 32 x 32 walk; 127 -> H_pad 128; an odd A
    f  64 x 4 = 256 cells, H 128, (128, 128) / (128,), 8 axes    every maximum at once: the LDS plan of npb_ppo_seq.hip's header (158 368 B),
                                                                 A = 8 fills the head buffer; a buffer sized short of its plan overlaps the next
    g  51 x 5 = 255 cells, H 1, (1,) / (128,), 7 axes            a core of one unit: H_pad 4, three rows of W_hh in npd_ppo_back_onto<3>, a
                                                                 padded row read as live moves the carry; 255 -> 256 cells
    h  33 x 2 = 66 cells, H 31, (31, 32, 33) / (3, 2, 1), 1 axis three hidden layers on both sides of 32 behind a core: the nets' phase uses
                                                                 b2 .. b4, which the cell's phase then reuses for r, z, n; one axis

Types are mixed per row: ``obs``, ``act`` (the controls' input type) and ``adv`` / ``ret`` are each float64 in four rows and float32 in
four.  The doubles are not floats: every float32 draw times (1 + 1e-9 u), |u| <= 1, so a kernel that read a double branch as floats, or
narrowed ``act`` or ``adv`` before the epilogue's double arithmetic, moves the ratio by far more than 4 ulp of a double.  The features are
narrowed to float32 first, by the kernel and by the statement: the perturbed ``obs`` give the bits of their float32 roundings.  Half the
rows run with clip_vf = 0.2.

TIME'S EDGES (recurrent_train_support.edges): a restart in front of the last slot and in front of slot 1, poisoned cells at slot 0 of plant
31 and at the last slot of plant 32 (the tile seam), two poisoned slots in a row on the last plant of the ragged tile, a cell restarted and
poisoned, a cell poisoned and skipped, and for float64 features a 1e300, which only the narrowing makes an infinity.  A sweep that read the
restart word of slot s for slot s - 1, dropped the +0.0 behind a poisoned cell, or counted a cell twice fails by bits or by the count.
t = 1 runs the ``s == 0`` branches alone (no carry, no restart word read); t = 2 has one carry and its restart in front of the last slot.

The host half of every input is built by the functions below from seeds alone, so tests/test_recurrent_shapes_cpu.py holds the statement
to float64 autograd at these shapes and asserts the CONDITIONS the tests here rest on (both branches of every gate's clamp and of the clip
taken, the skipped count, the restarts where they were planted) without a GPU; the tests here assert them again on what they ran."""
import functools

import numpy as np
import pytest
import torch

from nuclear_sim_amd import ppo, recurrent
from recurrent_train_support import EDGE_PLANTS, CUT, autograd, bits, distance, edges, poisoned_cells, problem, statement
from segments_support import rollout_problem, segment_batch
from test_policy_gpu import F32, F64, _np, _same
from test_recurrent_train_gpu import HYPER, _batch, _hold, _setup
import test_segments_gpu as seg

pytestmark = pytest.mark.gpu

N32, N64 = np.float32, np.float64
TABLE = {  # C, K, H, actor, critic, axes, obs, act, adv and ret, clip_vf
    "a": (16, 4, 64, (64,), (64,), 2, N32, N64, N64, 0.2),
    "b": (16, 4, 65, (7,), (9,), 4, N64, N32, N32, 0.0),
    "c": (13, 5, 64, (7,), (9,), 3, N32, N64, N32, 0.2),
    "d": (16, 4, 5, (7,), (65,), 3, N32, N32, N64, 0.0),
    "e": (25, 4, 127, (100, 96), (127,), 5, N64, N32, N64, 0.2),
    "f": (64, 4, 128, (128, 128), (128,), 8, N64, N64, N32, 0.0),
    "g": (51, 5, 1, (1,), (128,), 7, N32, N64, N32, 0.2),
    "h": (33, 2, 31, (31, 32, 33), (3, 2, 1), 1, N64, N32, N64, 0.0),
}
ROWS = sorted(TABLE)
SEED = {"a": 201, "b": 202, "c": 203, "d": 204, "e": 205, "f": 206, "g": 207, "h": 208}
TORCH = {N32: F32, N64: F64}
# t, count, plants_per_chain.  (4, 70, 64): two chains, the last tile 6 wide.  Rows e and f take (3, 33, 32) in its place: the numpy statement
# costs seconds a call there.  (1, 33, 32): no carry at all.  (2, 33, 32), rows b and g: one carry
MAIN = {row: (3, 33, 32) if row in "ef" else (4, 70, 64) for row in ROWS}
RUNS = [(row, run) for row in ROWS for run in [MAIN[row], (1, 33, 32)] + ([(2, 33, 32)] if row in "bg" else [])]
SEGMENT_ROWS = {"b": (70, 64), "d": (70, 64), "f": (33, 32), "g": (70, 64)}      # row: segments of the minibatch, chain
T6, N_ROLLOUT = 6, 35
BAND = (0.1, 0.9)


# ---------------------------------------------------------------------------------------------------------------- the inputs, host only
def retype(P, row):
    """the row's types, in place: a float64 tensor is its float32 draw times (1 + 1e-9 u), |u| <= 1 -- a double that is no float, and
    whose narrowing gives the draw back (a float's half ulp is a relative 3e-8 at the least).  NaNs stay NaNs"""
    rng = np.random.default_rng(7000 + SEED[row])
    for names, dtype in zip((("obs",), ("act",), ("adv", "ret")), TABLE[row][6:9]):
        for name in names:
            if dtype == N64:
                P[name] = P[name].astype(N64) * (1.0 + 1e-9 * rng.uniform(-1.0, 1.0, P[name].shape))
    return P


@functools.lru_cache(maxsize=None)
def _table_problem(row, t, count, gates, activation):
    C, K, H, actor, critic, A = TABLE[row][:6]
    P = retype(problem(SEED[row], t, count, C * K, H, A, actor, critic, gates, activation, special=False), row)
    if t >= 3:
        skipped = edges(P)
    elif t == 2:      # the one carry there is: cut in front of the last slot for one plant, dropped behind a poisoned slot 0 for another
        P["ended"][0, EDGE_PLANTS["cut"]] |= CUT
        P["obs"][0, 31, 0] = np.nan
        skipped = 1
    else:
        P["first"][3] = 0.0
        skipped = 0
    return P, skipped


def table_problem(row, t, count, gates="hard", activation="relu"):
    """``(P, skipped)``: the row's problem of t slots by count plants in the row's types with its edge cells, and the skipped count they
    make.  The arrays are shared between the callers: nobody writes into them (``_setup`` replaces P["theta"], in the caller's own dict)"""
    P, skipped = _table_problem(row, t, count, gates, activation)
    return dict(P), skipped


@functools.lru_cache(maxsize=None)
def _table_rollout(row, every, gates, activation):
    C, K, H, actor, critic, A = TABLE[row][:6]
    return retype(rollout_problem(300 + SEED[row] + every, T6, N_ROLLOUT, C * K, H, A, actor, critic, gates, activation, every), row)


def table_rollout(row, every, gates="hard", activation="relu"):
    """the row's rollout problem (segments_support.rollout_problem: T = 6 slots by 35 plants, its special cells laid against the segment
    boundaries) in the row's types; the stored states are those of the float32 roundings, which the narrowing gives back.  Shared as
    ``table_problem``'s are"""
    return dict(_table_rollout(row, every, gates, activation))


def gate_shares(out, P):
    """the share of exact zeros among the r, z and n gate deltas (``gradient(..., keep=True)``) of the cells that are not poisoned: with
    hard gates the clamped branches give +0.0 and the open ones do not"""
    live, H = ~poisoned_cells(P), P["core"]
    d = out["delta_i"][live]
    return [float((d[:, g * H:(g + 1) * H] == 0).mean()) for g in range(3)]


def conditions(P, skipped, out, band=True):
    """what every run rests on, of the statement's outputs ``out`` (``keep=True`` where ``band``): the skipped count, the restarts where
    ``edges`` planted them, and (the main runs) both branches of every gate's clamp and of the clip taken"""
    t, count = P["t"], P["count"]
    assert out["stats"]["skipped"] == skipped and out["stats"]["count"] == t * count
    fresh = recurrent.restarts(P["episode"], P["ended"])
    if t >= 2:
        assert fresh[1, EDGE_PLANTS["cut"]]
    if t >= 3:
        assert fresh[t - 1, EDGE_PLANTS["episode"]] and fresh[2, EDGE_PLANTS["restarted"]] and fresh.sum() == 3
    if band:
        shares = gate_shares(out, P)
        print("exact zeros among the r, z, n gate deltas: %.2f %.2f %.2f; clip fraction %.2f" % (*shares, out["stats"]["clip_fraction"]))
        assert all(BAND[0] <= s <= BAND[1] for s in shares), shares
        assert 0.0 < out["stats"]["clip_fraction"] < 1.0


# ---------------------------------------------------------------------------------------------------------------- the device's side
def _table_setup(row, t, count, gates="hard", activation="relu"):
    C, K, H, actor, critic = TABLE[row][:5]
    P, skipped = table_problem(row, t, count, gates, activation)
    env, P = _setup(0, count, C, K, H, actor, critic, gates, activation, cdtype=TORCH[TABLE[row][7]], P=P)
    return env, P, skipped


def _poisoned_rows(P, got, skipped):
    """on the device's outputs: the skipped count, the poisoned cells' +0.0 h' and NaN value, and a gradient that is finite and moves
    both the core and the nets"""
    bad = poisoned_cells(P)
    hidden = _np(got["hidden"])
    assert not bits(hidden[bad]).any() and np.isnan(_np(got["value_new"])[bad]).all() and np.isfinite(hidden).all()
    assert hidden[~bad].any(axis=1).mean() > 0.9
    assert _np(got["stats"])[ppo.STATS.index("skipped")] == skipped and (skipped == 0) == (not bad.any())
    _moves(P, _np(got["grad"]))


def _moves(P, grad):
    n_core = recurrent.core_size(P["cells"], P["core"])
    assert np.isfinite(grad).all() and grad[:n_core].any() and grad[n_core:-2 * P["n_axes"]].any()


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("row, run", RUNS, ids=["%s-t%d-%d" % (row, run[0], run[1]) for row, run in RUNS])
def test_hard_gates_and_relu_nets_bit_for_bit_at_the_table(row, run):
    t, count, chain = run
    env, P, skipped = _table_setup(row, t, count)
    assert P["obs"].dtype == TABLE[row][6] and P["act"].dtype == TABLE[row][7] and P["adv"].dtype == P["ret"].dtype == TABLE[row][8]
    main = run == MAIN[row]
    got, want = _hold(env, P, chain, keep=main, clip_vf=TABLE[row][9])
    conditions(P, skipped, want, band=main)
    _poisoned_rows(P, got, skipped)
    if t == 1:
        assert not P["first"][3].any() and P["first"][2].any()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 2
def _segment_setup(row, every, gates="hard", activation="relu"):
    C, K, H, actor, critic = TABLE[row][:5]
    R = table_rollout(row, every, gates, activation)
    return seg._setup(0, N_ROLLOUT, every, C, K, H, actor, critic, gates, activation, cdtype=TORCH[TABLE[row][7]], R=R)


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("row", sorted(SEGMENT_ROWS))
def test_segments_at_the_table(row, every):
    count, chain = SEGMENT_ROWS[row]
    env, R = _segment_setup(row, every)
    Q = segment_batch(R, seg._ids(R, count, seed=every))
    assert Q["count"] == count and Q["obs"].dtype == TABLE[row][6] and Q["act"].dtype == TABLE[row][7] and Q["adv"].dtype == TABLE[row][8]
    got, want = seg._hold(env, R, Q, chain, clip_vf=TABLE[row][9])
    assert want["stats"]["skipped"] == 2 and want["stats"]["count"] == every * count
    S = R["starts"]
    assert not S[1, 1].any() and not S[1, 4].any() and S[1, 0].any()      # the boundary restart and the poisoned last slot of segment 0
    j = {int(g): k for k, g in enumerate(Q["index"])}
    hidden = _np(got["hidden"])
    assert np.isnan(_np(got["value_new"])[every - 1, j[4]]) and not bits(hidden[every - 1, j[4]]).any()      # the poisoned cell and its h'
    s5, g5 = (T6 - 2) % every, 5 + ((T6 - 2) // every) * N_ROLLOUT
    assert np.isnan(_np(got["ratio"])[s5, j[g5]]) and hidden[s5, j[g5]].any()      # the skipped one still ran
    _moves(R, _np(got["grad"]))
    env.close()


def test_a_segment_batch_is_the_whole_sequence_call_by_bits_one_past_the_small_build():
    """row b, device against device, soft gates and tanh nets: every = 3 against the whole-sequence call on the hand-made problem whose
    'rollout' is [L][the segments] and whose first is the stored states gathered"""
    kw = dict(HYPER, clip_vf=0.2)
    env, R = _segment_setup("b", 3, "soft", "tanh")
    Q = segment_batch(R, seg._ids(R, 70, seed=2))
    a = env.policy_grad_sequences(seg._batch(env, R, Q), plants_per_chain=64, diagnostics=True, **kw)
    made = {k: torch.as_tensor(Q[k]).to(env.device) for k in ("obs", "act", "logp_old", "adv", "ret", "value_old", "episode", "ended", "first")}
    b = env.policy_grad_sequences(made, plants_per_chain=64, diagnostics=True, **kw)
    for k in seg.KEYS:
        _same(a[k], b[k], k)
    assert _np(a["stats"])[ppo.STATS.index("skipped")] == 2
    _moves(R, _np(a["grad"]))
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_a_workgroup_that_takes_several_chains_but_not_all():
    """row a, 150 plants in chains of 32: five chains, the last of 22 plants.  max_blocks = 2 gives workgroup 0 the chains 0, 2, 4 and
    workgroup 1 the chains 1, 3; 3 gives 0 and 3, 1 and 4, and 2 alone; 0 a workgroup a chain.  The running sums and the `first` flag are
    per chain: no bit may differ, and the launch of a workgroup a chain holds the statement's"""
    env, P, skipped = _table_setup("a", 3, 150)
    batch = _batch(env, P)
    kw = dict(HYPER, clip_vf=TABLE["a"][9])
    got, want = _hold(env, P, 32, batch, keep=True, clip_vf=TABLE["a"][9])
    conditions(P, skipped, want)
    _poisoned_rows(P, got, skipped)
    for blocks in (2, 3):
        out = env.policy_grad_sequences(batch, plants_per_chain=32, max_blocks=blocks, diagnostics=True, **kw)
        for k in seg.KEYS:
            _same(out[k], got[k], (blocks, k))
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("row", ["b", "e"])
def test_soft_gates_and_tanh_nets_within_8_times_the_statements_distance_at_the_table(row):
    """the soft branch of the cell's backward pass in the large build and at a padded width (H 65 -> 68, 127 -> 128)"""
    t, count, chain = MAIN[row]
    env, P, skipped = _table_setup(row, t, count, "soft", "tanh")
    hyper = dict(HYPER, max_grad_norm=0.0)
    got = env.policy_grad_sequences(_batch(env, P), plants_per_chain=chain, diagnostics=True, **hyper)
    own = statement(P, plants_per_chain=chain, **hyper)
    g64 = autograd(P, ent_coef=HYPER["ent_coef"])
    mine, yard = distance(_np(got["grad"]), g64), distance(own["grad"], g64)
    print("row %s, pooled distance from float64: the device %.3e, the statement %.3e, factor %.2f" % (row, mine, yard, mine / yard))
    assert mine <= 8 * yard
    assert own["stats"]["skipped"] == skipped
    _poisoned_rows(P, got, skipped)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("row", ["c", "g"])
def test_shard_sums_of_sequences_bit_for_bit(row):
    """a shard's vector of doubles against recurrent.shard_sums fed the device's ratio, the seeds divided by a count that is not the
    batch's own"""
    t, count, chain = MAIN[row]
    env, P, skipped = _table_setup(row, t, count)
    batch, clip_vf = _batch(env, P), TABLE[row][9]
    total = t * count + 123
    got = env.policy_grad_sequences(batch, plants_per_chain=chain, diagnostics=True, clip_vf=clip_vf, **HYPER)
    _poisoned_rows(P, got, skipped)
    ratio = _np(got["ratio"])
    vec = env.policy_shard_sums_sequences(batch, total, plants_per_chain=chain, clip_vf=clip_vf)
    want = statement(P, recurrent.shard_sums, count_total=total, plants_per_chain=chain, ratio=ratio, value_old=P["value_old"], clip_vf=clip_vf)
    _same(vec, want, "the shard's vector")
    own = statement(P, recurrent.shard_sums, count_total=t * count, plants_per_chain=chain, ratio=ratio, value_old=P["value_old"], clip_vf=clip_vf)
    n_core, n_w = recurrent.core_size(P["cells"], P["core"]), P["theta"].size - 2 * P["n_axes"]
    assert not np.array_equal(own[:n_w], want[:n_w])      # (the divisor does reach the seeds)
    assert np.isfinite(want).all() and want[:n_core].any() and want[n_core:n_w].any() and want[n_w + ppo.SHARD_ROWS.index("skipped")] == skipped
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 6
STORED = [(33, 13, 5, F64, 65, (33, 17), (7,)), (64, 64, 4, F32, 128, (128, 128), (128,))]


@pytest.mark.parametrize("n, C, K, fdtype, H, actor, critic", STORED, ids=["33-65-65-f64", "64-256-128"])
def test_the_stored_states_at_the_large_shapes_after_a_real_collect(n, C, K, fdtype, H, actor, critic):
    """every = 3 under autoreset with a step limit of 3 from a start bank, some plants reset before the rollout: the recording
    (npb_policy_core_segments) and the refresh (npb_segment_starts_kernel's large build; its double branch in the first case) against
    recurrent.starts by bits, under the collecting parameters and under perturbed ones; then one gathered segment minibatch through the
    gradient kernel against recurrent.gradient_segments"""
    L, A = 3, 3
    env = seg._collecting(n, 3, every=L, H=H, fdtype=fdtype, C=C, K=K, actor=actor, critic=critic)
    seg._steps(env, T6)
    seg._advantages(env)
    S = env.policy_spec()
    r, rh = env.rollout(), env.policy_rollout_hidden()
    assert r["t"] == T6 and rh["every"] == L and rh["starts"].shape == (2, n, H) and r["obs"].dtype == fdtype
    obs, episode, ended, first = _np(r["obs"]), _np(r["episode"]), _np(r["ended"]), _np(rh["first"])
    recorded = _np(rh["starts"])
    fresh = recurrent.restarts(episode, ended)
    assert fresh[3].any() and not fresh[3].all() and (fresh[2] | fresh[4] | fresh[5]).any()      # restarts on the boundary, and inside segments
    assert not (recorded == seg.SENTINEL).any() and not recorded[1][fresh[3]].any() and recorded[1][~fresh[3]].any(axis=1).all()
    _same(recorded, recurrent.starts(first, obs, episode, ended, seg._core_of(env), "hard", L), "the recorded states")
    # the refresh under the collecting parameters: row 1 again, row 0 not touched
    rh["starts"][0].fill_(seg.SENTINEL)
    rh["starts"][1].fill_(-seg.SENTINEL)
    env.policy_refresh_segments()
    now = _np(env.policy_rollout_hidden()["starts"])
    assert (now[0] == seg.SENTINEL).all()
    _same(now[1], recorded[1], "the refresh before any update")
    # under other parameters: every weight of the core moved by a relative 1e-3 draw
    theta = _np(env.policy_theta())
    n_core = recurrent.core_size(C * K, H)
    theta[:n_core] *= (1.0 + 1e-3 * np.random.default_rng(n).standard_normal(n_core)).astype(np.float32)
    env.policy_load(theta)
    rh["starts"].copy_(torch.as_tensor(recorded))
    env.policy_refresh_segments()
    theta = _np(env.policy_theta())
    fresh_states = _np(env.policy_rollout_hidden()["starts"])
    _same(fresh_states, recurrent.starts(first, obs, episode, ended, seg._core_of(env), "hard", L), "the refreshed states under the new theta")
    assert not np.array_equal(fresh_states[1], recorded[1])
    # one gathered segment minibatch under those parameters and states
    B, kw = 50, dict(HYPER, clip_vf=0.2)
    batch = next(iter(env.rollout_minibatches(B, 1, seed=3, unit="segment")))
    assert batch["every"] == L and batch["obs"].dtype == fdtype and batch["index"].numel() == B
    got = env.policy_grad_sequences(batch, plants_per_chain=32, diagnostics=True, **kw)
    extra = _np(batch["extra"])
    want = recurrent.gradient_segments(theta, S["cells"], A, S["actor"], S["critic"], "relu", S["core"], "hard", _np(batch["obs"]).reshape(L, B, -1),
                                       _np(batch["act"]), extra[..., 1], _np(batch["adv"]), _np(batch["ret"]), episode, ended, fresh_states,
                                       _np(batch["index"]), env.n, L, ratio=_np(got["ratio"]), value_old=extra[..., 0], **kw)
    _same(got["grad"], want["grad"], "grad of a gathered segment minibatch"); _same(got["hidden"], want["hidden"], "hidden")
    _same(got["logp_new"], want["logp_new"], "logp_new"); _same(got["value_new"], want["value_new"], "value_new")
    _same(got["stats"], np.array([want["stats"][k] for k in ppo.STATS]), "stats")
    ratio = _np(got["ratio"])
    assert want["stats"]["count"] == L * B and (ratio[np.isfinite(ratio)] != 1.0).any()      # (the parameters did move)
    _moves(dict(cells=C * K, core=H, n_axes=A), _np(got["grad"]))
    env.close()
