"""The policy on the device, stated once in numpy: what ``env.set_policy`` runs in front of every step (npb_set_policy,
nuclear_sim_amd/csrc/npb_policy.hip).  Host only.  This statement is the contract; the device gives its bits for every n, storage type
and launch geometry -- with ONE licensed difference, the float ``tanh`` (below).

THE NETS.  A diagonal-Gaussian actor and a critic, two separate MLPs of 1 to 3 hidden layers each, widths 1 .. 128 chosen per net, one
activation (``"relu"`` or ``"tanh"``) for both.  The input is a plant's features stack flattened, K * C cells (at most 256).  The actor's
head has A outputs, one per controls axis (1 .. 8): the means.  The critic's head has one: the value.

THE PARAMETERS are one flat float32 vector ``theta``: the actor's layers, then the critic's, then ``log_std[A]``, then ``std[A]``; each
layer ``W[out][in]`` row-major (``nn.Linear.weight``) and then ``b[out]``.  ``pack`` and ``unpack`` state it.  ``std`` is the CALLER's
``exp(log_std)``: the device takes no exponential.

THE INPUT is read as float32: a float32 tensor as it is, a float64 one narrowed, round to nearest even.

ONE LAYER (``layer``).  For output j: ``acc = b[j]``, then for k ascending ``acc = fmaf(x[k], W[j][k], acc)`` in float32 -- a single
rounding per step, what ``v_fma_f32`` and the f32 matrix cores both give.  k is extended with +0.0 cells and +0.0 weights to a multiple of 4
(a kernel that pads K does this statement's arithmetic, signed zeros included: the extension turns an accumulator of -0.0 into +0.0 and
changes nothing else).  A subnormal result or accumulator is outside the contract.  Hidden values are float32.
Numpy has no fmaf: ``fmaf`` emulates it.  Widen to float64, where the product is exact (24 + 24 bits); ``s = p + c`` with its exact error
``e`` by TwoSum; where ``e != 0`` and the last mantissa bit of ``s`` is 0, ``s`` moves one ulp towards the exact value (round to odd); then
narrow to float32.  Round to odd keeps the sticky information the second rounding needs: 53 >= 2 * 24 + 2.

THE ACTIVATION.  relu: ``acc > 0 ? acc : +0.0`` (a NaN gives +0.0).  tanh: ``float32(tanh(float64(acc)))`` here; the device uses its
float ``tanh`` (OpenCL bound: 5 ulp).  That is the one licensed difference; a relu net is reproduced bit for bit.

THE NOISE (``noise``, ``philox4x32``).  Philox4x32-10, key = the two halves of a 64-bit ``seed`` (low word first), counter =
``(first_plant + p, t & 0xffffffff, t >> 32, j)``; ``t`` is the policy's draw counter (uint64, advanced by every sampling step); call j
serves axes 2j and 2j + 1.  From its four words ``u1 = (w0 * 2^20 + (w1 >> 12) + 0.5) * 2^-52`` and ``u2`` likewise from w2, w3: exact, in
(0, 1).  ``r = sqrt(-2 * log(u1))``, ``th = 6.283185307179586 * u2``, ``z0 = r * cos(th)``, ``z1 = r * sin(th)``, in double.  |z| <=
sqrt(2 * 53 * ln 2) < 8.58.  Deterministic: nothing is drawn, z = 0 and t does not advance.

THE OUTPUTS (``outputs``), in double, every operation rounded on its own:

    a[i]  = (double)mean[i] + (double)std[i] * z[i]          narrowed to the controls' input type, round to nearest even
    lp    = -(A * 0.9189385332046727);  for i ascending  lp = (lp - 0.5 * (z[i] * z[i])) - (double)log_std[i]
    value = the critic's float;  logp = (float)lp

``logp`` is the density of the UNROUNDED action mean + std * z, not of the float the controls read.

NaN AND INFINITY.  A plant with a NaN or infinite feature (after the narrowing) gets THE quiet NaN in every output -- every action,
value and logp -- whatever its nets would have made of it (a relu turns a NaN into +0.0), and touches no other plant."""
import numpy as np

CELLS_MAX, HIDDEN_MAX, WIDTH_MAX, AXES_MAX = 256, 3, 128, 8
ACTIVATIONS = {"relu": 0, "tanh": 1}
HALF_LOG_2PI = 0.9189385332046727
TWO_PI = 6.283185307179586
Z_MAX = 8.58
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def fmaf(a, b, c):
    """float32 fma(a, b, c) with a single rounding, elementwise (the module docstring says how)"""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b                       # exact
        s = p + c
        bb = s - p                      # TwoSum (Knuth): s + e == p + c exactly
        e = (p - (s - bb)) + (c - bb)
        s = np.array(s, dtype=np.float64)      # (a 0-d result becomes an array the masks below can write)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0.0) & ((s.view(np.uint64) & np.uint64(1)) == 0)
        if fix.any():
            toward = np.where((e > 0.0) == (s > 0.0), 1, -1).astype(np.int64)      # one ulp away from or towards zero
            # s == 0 with e != 0 cannot happen: p + c rounds to 0 only when it is 0
            bits = s.view(np.int64)
            bits[fix] += toward[fix]
        return s.astype(np.float32)


def sizes(cells, n_axes, actor, critic):
    """[(in, out)] of every layer, the actor's then the critic's, heads included"""
    def net(hidden, head):
        dims = [int(cells)] + [int(w) for w in hidden] + [head]
        return list(zip(dims[:-1], dims[1:]))
    return net(actor, int(n_axes)), net(critic, 1)


def check(cells, n_axes, actor, critic, activation):
    """refuse what npb_policy_check refuses of the shapes, by name"""
    if not 1 <= int(cells) <= CELLS_MAX:
        raise ValueError("a policy reads 1 to %d feature cells, not %r" % (CELLS_MAX, cells))
    if not 1 <= int(n_axes) <= AXES_MAX:
        raise ValueError("a policy writes 1 to %d axes, not %r" % (AXES_MAX, n_axes))
    for who, hidden in (("actor", actor), ("critic", critic)):
        if not 1 <= len(hidden) <= HIDDEN_MAX:
            raise ValueError("the %s has 1 to %d hidden layers, not %d" % (who, HIDDEN_MAX, len(hidden)))
        for w in hidden:
            if not 1 <= int(w) <= WIDTH_MAX:
                raise ValueError("a hidden layer of the %s is 1 to %d wide, not %r" % (who, WIDTH_MAX, w))
    if activation not in ACTIVATIONS:
        raise ValueError("the activation is 'relu' or 'tanh', not %r" % (activation,))


def theta_size(cells, n_axes, actor, critic):
    a, c = sizes(cells, n_axes, actor, critic)
    return sum(i * o + o for i, o in a + c) + 2 * int(n_axes)


def pack(actor, critic, log_std, std=None):
    """``theta`` of an actor and a critic, each a list of ``(W[out][in], b[out])``, heads last, and ``log_std[A]``; ``std`` defaults to
    ``exp(log_std)`` formed in float32"""
    log_std = np.asarray(log_std, dtype=np.float32).reshape(-1)
    std = np.exp(log_std).astype(np.float32) if std is None else np.asarray(std, dtype=np.float32).reshape(-1)
    if std.shape != log_std.shape:
        raise ValueError("std and log_std differ in length")
    parts, width = [], None
    for net in (actor, critic):
        width = None
        for W, b in net:
            W, b = np.asarray(W, dtype=np.float32), np.asarray(b, dtype=np.float32).reshape(-1)
            if W.ndim != 2 or b.shape != (W.shape[0],) or (width is not None and W.shape[1] != width):
                raise ValueError("a layer is W[out][in] and b[out], its `in` the width of the layer before")
            parts += [W.reshape(-1), b]
            width = W.shape[0]
    if len(actor[-1][1]) != len(log_std) or len(critic[-1][1]) != 1 or np.asarray(actor[0][0]).shape[1] != np.asarray(critic[0][0]).shape[1]:
        raise ValueError("the actor's head has len(log_std) outputs, the critic's one, and both nets read the same cells")
    return np.concatenate(parts + [log_std, std]).astype(np.float32)


def unpack(theta, cells, n_axes, actor, critic):
    """the inverse: ``(actor, critic, log_std, std)`` of a ``theta`` with these hidden widths"""
    theta = np.asarray(theta, dtype=np.float32).reshape(-1)
    if theta.size != theta_size(cells, n_axes, actor, critic):
        raise ValueError("theta has %d elements, these shapes take %d" % (theta.size, theta_size(cells, n_axes, actor, critic)))
    at = 0
    nets = []
    for dims in sizes(cells, n_axes, actor, critic):
        net = []
        for i, o in dims:
            W = theta[at:at + i * o].reshape(o, i); at += i * o
            b = theta[at:at + o]; at += o
            net.append((W, b))
        nets.append(net)
    A = int(n_axes)
    return nets[0], nets[1], theta[at:at + A], theta[at + A:at + 2 * A]


def layer(x, W, b):
    """one layer before its activation: x float32 [n, in] -> float32 [n, out], the fmaf chain with k extended to a multiple of 4"""
    x, W = np.asarray(x, dtype=np.float32), np.asarray(W, dtype=np.float32)
    n, K = x.shape
    pad = -K % 4
    if pad:
        x = np.concatenate([x, np.zeros((n, pad), np.float32)], axis=1)
        W = np.concatenate([W, np.zeros((W.shape[0], pad), np.float32)], axis=1)
    acc = np.broadcast_to(np.asarray(b, dtype=np.float32), (n, W.shape[0])).copy()
    for k in range(K + pad):
        acc = fmaf(x[:, k:k + 1], W[None, :, k], acc)
    return acc


def activate(acc, activation):
    if activation == "relu":
        return np.where(acc > 0, acc, np.float32(0.0)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return np.tanh(acc.astype(np.float64)).astype(np.float32)


def forward(net, x, activation):
    """a net's head outputs, float32 [n, out], of float32 (or narrowed float64) rows x [n, cells]"""
    with np.errstate(over="ignore", invalid="ignore"):
        h = np.asarray(x).astype(np.float32).reshape(len(x), -1)
    for W, b in net[:-1]:
        h = activate(layer(h, W, b), activation)
    return layer(h, *net[-1])


def philox4x32(counter, key, rounds=10):
    """Philox4x32: counter uint32 [..., 4], key uint32 [..., 2] (broadcast) -> uint32 [..., 4]"""
    c = [np.asarray(counter, dtype=np.uint32)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key, dtype=np.uint32)[..., i].astype(np.uint64) for i in range(2)]
    lo32 = np.uint64(0xFFFFFFFF)
    for _ in range(rounds):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & lo32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & lo32]
        k = [(k[0] + np.uint64(_W0)) & lo32, (k[1] + np.uint64(_W1)) & lo32]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def noise_words(seed, t, n, n_axes, first_plant=0):
    """the words of draw t: uint32 [n, ceil(A / 2), 4]"""
    seed, t = int(seed) & (2 ** 64 - 1), int(t) & (2 ** 64 - 1)
    J = (int(n_axes) + 1) // 2
    counter = np.zeros((n, J, 4), dtype=np.uint32)
    counter[..., 0] = ((int(first_plant) + np.arange(n, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None]
    counter[..., 1], counter[..., 2] = t & 0xFFFFFFFF, t >> 32
    counter[..., 3] = np.arange(J, dtype=np.uint32)[None, :]
    return philox4x32(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32))


def noise_from_words(words, n_axes):
    """z float64 [n, A] of the words [n, J, 4]"""
    w = np.asarray(words, dtype=np.uint32).astype(np.float64)
    hi = np.asarray(words, dtype=np.uint32) >> np.uint32(12)
    u1 = (w[..., 0] * 1048576.0 + hi[..., 1].astype(np.float64) + 0.5) * 2.0 ** -52
    u2 = (w[..., 2] * 1048576.0 + hi[..., 3].astype(np.float64) + 0.5) * 2.0 ** -52
    r = np.sqrt(-2.0 * np.log(u1))
    th = TWO_PI * u2
    z = np.stack([r * np.cos(th), r * np.sin(th)], axis=-1).reshape(len(w), -1)
    return z[:, :int(n_axes)]


def noise(seed, t, n, n_axes, first_plant=0):
    """z of draw t: float64 [n, A]"""
    return noise_from_words(noise_words(seed, t, n, n_axes, first_plant), n_axes)


def outputs(mean, value, log_std, std, z, x, act_dtype=np.float32):
    """``(action [n, A] of act_dtype, value float32 [n], logp float32 [n])`` of the heads' floats, the noise z [n, A] (zeros when
    deterministic) and the rows x the nets read (for the plants that get NaN)"""
    mean, z = np.asarray(mean, dtype=np.float32), np.asarray(z, dtype=np.float64)
    n, A = mean.shape
    log_std, std = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (log_std, std))
    with np.errstate(invalid="ignore", over="ignore"):
        a = mean.astype(np.float64) + std[None, :] * z
        lp = np.full(n, -(A * HALF_LOG_2PI))
        for i in range(A):
            lp = (lp - 0.5 * (z[:, i] * z[:, i])) - log_std[i]
        a, lp = a.astype(act_dtype), lp.astype(np.float32)
        v = np.asarray(value, dtype=np.float32).reshape(n).copy()
        bad = ~np.isfinite(np.asarray(x).astype(np.float32).reshape(n, -1)).all(axis=1)
    a[bad], v[bad], lp[bad] = np.nan, np.nan, np.nan
    return a, v, lp


class Policy:
    """What the device keeps: the shapes, ``theta``, the seed and the draw counter ``t``.  ``step(x)`` is one step's launch: ``(action,
    value, logp)`` of the features x [n, K, C] (or [n, K * C]); ``values(x)`` is npb_policy_values."""

    def __init__(self, cells, n_axes, actor, critic, activation="tanh", seed=0, deterministic=False, first_plant=0, act_dtype=np.float32):
        check(cells, n_axes, actor, critic, activation)
        self.cells, self.n_axes, self.actor, self.critic = int(cells), int(n_axes), tuple(int(w) for w in actor), tuple(int(w) for w in critic)
        self.activation, self.seed, self.deterministic, self.first_plant = activation, int(seed), bool(deterministic), int(first_plant)
        self.act_dtype, self.t, self.theta = act_dtype, 0, None

    def load(self, theta):
        self.theta = np.array(theta, dtype=np.float32).reshape(-1)
        self.nets = unpack(self.theta, self.cells, self.n_axes, self.actor, self.critic)

    def values(self, x):
        x = np.asarray(x)
        x = x.reshape(len(x), -1)
        v = forward(self.nets[1], x, self.activation)[:, 0].copy()
        with np.errstate(over="ignore", invalid="ignore"):
            v[~np.isfinite(x.astype(np.float32)).all(axis=1)] = np.nan
        return v

    def step(self, x, z=None):
        """one step; ``z`` given: the device's own draw in place of the statement's (what the tests feed back)"""
        x = np.asarray(x)
        x = x.reshape(len(x), -1)
        actor, critic, log_std, std = self.nets
        if self.deterministic:
            z = np.zeros((len(x), self.n_axes))
        else:
            if z is None:
                z = noise(self.seed, self.t, len(x), self.n_axes, self.first_plant)
            self.t += 1
        return outputs(forward(actor, x, self.activation), forward(critic, x, self.activation)[:, 0], log_std, std, z, x, self.act_dtype)
