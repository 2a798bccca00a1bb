"""Geometries, weight sets, partial-sum regimes and float64 references for the fp32 side kernels of osconv.hip, stage by stage (numpy + torch,
no GPU, no engine): the OSConv weight chain  partial -> v1 -> v2 -> att -> weight image (direct and Winograd-y order), the RCAN SE gate and
the pooled channel sums.  v1, v2 and att are observable between the stages, so each stage is held to a PER-ELEMENT bound relative to that
element's own magnitude sum S = sum |term|, evaluated in float64 on what the launch itself read back from the stage before
(tests/range_cases.py and tests/satu_cases.py do the same for the conv and SATU kernels).  tests/test_osconv_cases.py checks this module on
the CPU, tests/test_gpu_osconv_chain.py holds the kernels to it.

u = 2^-24 (satu_cases.U24) is the unit roundoff of fp32 and gamma(n) = n u / (1 - n u) the usual bound of n chained roundings: a sum of
terms each of which passes through at most n rounded operations errs by <= gamma(n) S, whatever the data (an FMA rounds once where a product
and an add round twice: the count below is the larger one).  Adding to an accumulator that is still 0 is exact but counted all the same.
No bound below was measured; worst-case error is NOT propagated from stage to stage (at cin = 320 that allows 0.05 on logits of 0.5, and
says nothing), only through a value the kernel keeps in LDS and never writes out: the pooled mean, the hidden vector `a`, the SE gate's z.

Pooled mean (osconv_l1_kernel, osconv_route_in_workgroup).  Row b of the partials goes to slice b % 32; a slice is a chain of ceil(nblk / 32)
adds; the 32 slices are added in order; one multiply by inv_n:  |mean - exact| <= gamma(ceil(nblk / 32) + 32 + 1) S,  S = inv_n sum_b |partial|.
The SE gate has 16 slices: gamma(ceil(nblk / 16) + 16 + 1).  channel_sums_kernel with PL = 1024 / src_ch pixel lanes over a block of `per`
pixels: a chain of ceil(per / PL) adds per lane, then the PL lanes in order: gamma(ceil(per / PL) + PL).  Integer data whose sums stay below
2^24 comes out bit for bit (every partial sum is an integer fp32 holds).

A wave_dot-ordered row of n columns plus its bias (layers 1 and 2, the fc rows, the SE gate's first layer): lane l chains its q = ceil(n / 64)
products w[c] v[c], c = l + 64 j; a 6-level butterfly adds the lanes; the bias is added:  1 product + q adds + 6 + 1 = q + 8 roundings,
|got - exact| <= gamma(q + 8) S,  S = sum |w v| + |b|.  ReLU is 1-Lipschitz and exact.  A dropped column is ~ 1 / n of S, thousands of bounds.
  * v1 (from the partials): the row reads the kernel's own mean m^ from LDS, |m^ - m| <= e_m (above):
        |v1 - exact| <= gamma(q + 8) (|w| (|v0| + e_v0) + |b|) + |w| e_v0,     e_v0 = (0, 0, e_m): the two scales are exact inputs.
  * v2 (from the launch's v1): gamma(ceil(2 cin / 64) + 8) S.
  * a = ReLU(dot(fc, v2) bn_scale + bn_shift) (from the launch's v2): the dot without a bias is q + 7, then one multiply and one add:
        e_a = gamma(q + 9) S_a,   S_a = |bn_scale| sum |fc v2| + |bn_shift|.   `a` stays in LDS.

The heads.  logit_i = sum_k G[i][k] a[k] + b_i is a sequential chain of `hidden` products and adds plus the bias, hidden + 1 roundings per term
(the second gate loop of ngate > 512 runs the same order), from the kernel's a^:
        e_l = gamma(hidden + 1) (|G| (a + e_a) + |b|) + |G| e_a.
Sigmoid (ca, fa, sa): slope <= 1/4, and its own arithmetic 1 / (1 + expf(-v)) -- expf within 1 ulp as HIP documents it (2 u), a correctly rounded
add and divide -- errs by <= r (1 - r) 2 u + 2 u <= 3 u (the bound of test_gpu_satu_range._table64):   |gate - exact| <= e_l / 4 + 3 u.
At logits beyond +-88 expf overflows to inf or underflows to 0 and the gate is exactly 0 or 1: inside 3 u of the exact value.
Softmax (ka), temperature 1: m^ = max_k l^_k (one of the fp32 logits, a common shift: the softmax does not depend on it), d_k = fl(l^_k - m^),
p_k = expf(d_k), s = the K-term chain sum, ka_k = fl(p_k / s).  d_k differs from l_k - m^ by delta_k = e_l,k + u |d_k|, |d_k| <= spread_k +
2 max e_l with spread_k = max l - l_k; so p_k = exp(l_k - m^) (1 + theta_k), |theta_k| <= exp(delta_k) (1 + 2 u) - 1; all terms of s are positive, so s
is relative to within Theta = max theta and the chain's gamma(K); the divide rounds once:
        |ka_k - exact| <= ((1 + theta_k) (1 + u) / ((1 - Theta) (1 - gamma(K))) - 1) ka_k + FLOOR.
FLOOR = 2^-126: where exp(l_k - m^) is below fp32's normal range, p_k may be rounded as a subnormal or flushed to zero, an absolute error of less
than 2^-126, and s >= 1 (the maximum's term is exp(0) = 1) does not enlarge it.  The same floor is added to every image entry.

An image entry (from the launch's own att = ca | fa | sa | ka).  x = (sum_k ka_k W_k) ((fa sa) ca): a chain of K products and adds (K roundings per
term: its product and the K - 1 adds onto a non-zero accumulator), then fl(fa sa), fl(. ca) and the final product, 3 more:
        |x - exact| <= gamma(K + 3) T,   T = fa sa ca sum_k |ka_k W_k|.
(K + 3, not the 2 K of a first sketch: for knum = 1 there are 4 roundings, 2 K = 2 would have been wrong; for knum = 8 it is 11.)
The image holds hi = bf16(x), lo = bf16(x - hi), RNE both: |x - hi| <= 2^-8 |x| (bf16 has 8 significant bits: half a unit in the last place), so |x - hi - lo| <= 2^-8 |x - hi| <= 2^-16 |x|, and
|x| <= |exact| + gamma(K + 3) T; in all
        |decoded(hi + lo) - exact| <= gamma(K + 3) T (1 + 2^-16) + 2^-16 |exact| + FLOOR.
A lost lo half is up to 2^-8 |x|: 256 x the split term.  A missing bank is ka_k |W_k| gates, of the order of T itself.
Winograd-y entry: g_ky as above per tap row (the spatial gate sa[ky][kx] before the transform), U0 = g0, U3 = g2 (the same bound),
U1,2 = fl(0.5 fl(fl(g0 + g2) +- g1)): two adds (the halving is exact) on the computed g:
        |U - exact| <= (A (1 + 2^-16) + 2^-16 |exact|) + FLOOR,   A = 0.5 ((1 + gamma(2)) sum_ky gamma(K + 3) T_ky + gamma(2) sum_ky |g_ky|).
Zero and guard entries: T == 0 => both halves are 0 (every term has a zero factor); entries the pack index does not address (output channels
beyond cout in a 32 / 64 tile) are 0; nothing is written behind the image.
The fp16 images keep their existing criterion (tests/test_gpu_precision.py): within one fp16 ulp of the float64 value from the launch's gates.

SE gate (se_gate_block): nothing between the partials and the gate is observable, so the mean's and z's errors are carried through the two
small layers: z_r = ReLU(dot(w1[r], m^) + b1) in wave_dot order (q = ceil(c / 64); the preloaded form adds its two products first: the same
count), e_z = gamma(q + 8) (|w1| (|m| + e_m) + |b1|) + |w1| e_m;  logit_o = b2 + sum_k w2[o][k] z_k, a chain of cmid + 1 roundings,
e_l = gamma(cmid + 1) (|w2| (z + e_z) + |b2|) + |w2| e_z;  |gate - exact| <= e_l / 4 + 3 u.
se_scale_residual: out = fl(fl(r g) + x) or one FMA, from the kernel's own gate: |out - (r g + x)| <= u |r g| + u |r g + x| (two roundings at most).

Sharpness (test_osconv_cases.py on the fp32 restatements, test_gpu_osconv_chain.py on the device).  A defect moves an element by `moved`; the
element is DOMINATED where moved > 2 bound (then |got - exact| >= moved - |clean error| > bound as the clean error is inside the bound) and
UNTOUCHED where moved == 0.  The tests assert: at least 3 dominated elements, every one of them outside the bound, every untouched one inside.
"""
from functools import lru_cache

import numpy as np
import torch

from tests import range_cases as R
from tests.satu_cases import U24

F32 = np.float32
FLOOR = 2.0 ** -126
SPLIT = 2.0 ** -16
# (cin, cout, hidden, knum): the network's OSConvs at 64 and at 32 features, then the ABI's edges -- knum = 1; cout = 1 with hidden = 5; cout = 128 at
# hidden = 32 (the maximum); knum = 11 (the bank fallback loop) with hidden = 7; ngate = 529 (the second gate loop) at three 64-wide cout tiles.
# The fused path's scratch offset 2 cin + hidden + cout + 9 + knum is 1 modulo 4 for the network's and 1 or 3 for those edges; (16, 16, 2, 1) and
# (16, 16, 3, 2) add the residues 0 and 2.
NETWORK_GEOMS = ((64, 64, 16, 8), (192, 64, 16, 8), (320, 64, 20, 8), (32, 32, 16, 8), (96, 32, 16, 8), (160, 32, 16, 8))
EDGE_GEOMS = ((16, 16, 1, 1), (16, 1, 5, 2), (48, 128, 32, 8), (32, 64, 7, 11), (320, 192, 20, 8), (16, 16, 2, 1), (16, 16, 3, 2))
GEOMS = NETWORK_GEOMS + EDGE_GEOMS
NBLKS = (1, 31, 32, 33, 230)
SCALES = ((1.5, 4), (3.7, 3.7))
WEIGHT_SETS = ("synth", "probe", "dead", "sat", "uniform_k", "decades")
REGIMES = ("gauss", "mean50", "altsign", "integers", "zero", "lastblock", "decades")
OSC_PARTS, SE_PARTS = 32, 16
SE_GEOMS = ((64, 4), (32, 2), (16, 1), (4, 1), (128, 8), (64, 9), (128, 20))
SE_NBLKS = (1, 15, 16, 17, 230)


def gamma(n) -> float:
    return n * U24 / (1.0 - n * U24)


def ngate(geom) -> int:
    cin, cout, _, knum = geom
    return cin + cout + 9 + knum


def scratch_residue(geom) -> int:
    cin, cout, hidden, knum = geom
    return (2 * cin + hidden + cout + 9 + knum) % 4


def inv_scales(sc):
    return F32(1.0 / sc[0]), F32(1.0 / sc[1])


# ----------------------------------------------------------------------------- weight sets
def _f(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=F32)


@lru_cache(maxsize=None)
def weights(name: str, geom) -> dict:
    """Weight set `name` at geometry (cin, cout, hidden, knum): fp32 arrays l1_w [2 cin][cin + 2], l1_b, l2_w [cin][2 cin], l2_b, fc_w [hidden][cin],
    bn_scale, bn_shift, ch_w [cin][hidden], ch_b, fl_w [cout][hidden], fl_b, sp_w [9][hidden], sp_b, kn_w [knum][hidden], kn_b and
    bank [knum][cout][cin][3][3].  Shared: callers must not modify them."""
    cin, cout, hidden, knum = geom
    g = np.random.RandomState([WEIGHT_SETS.index(name), cin, cout, hidden, knum])
    n = lambda fan, *shape: g.standard_normal(shape) / np.sqrt(fan)      # noqa: E731
    w = dict(l1_w=n(cin + 2, 2 * cin, cin + 2), l1_b=0.1 * g.standard_normal(2 * cin), l2_w=n(2 * cin, cin, 2 * cin), l2_b=0.1 * g.standard_normal(cin),
             fc_w=n(cin, hidden, cin), bn_scale=g.uniform(0.5, 1.5, hidden), bn_shift=0.1 * g.standard_normal(hidden),
             ch_w=n(hidden, cin, hidden), ch_b=0.1 * g.standard_normal(cin), fl_w=n(hidden, cout, hidden), fl_b=0.1 * g.standard_normal(cout),
             sp_w=n(hidden, 9, hidden), sp_b=0.1 * g.standard_normal(9), kn_w=n(hidden, knum, hidden), kn_b=0.1 * g.standard_normal(knum),
             bank=n(cin * 9, knum, cout, cin, 3, 3))
    if name == "probe":
        w["l1_w"] = np.eye(2 * cin, cin + 2)
        w["l1_b"] = np.zeros(2 * cin)
    elif name == "dead":
        w["l1_b"] = np.full(2 * cin, -1e3)
    elif name == "sat":
        # `a` nearly data-independent (fc shrunk, bn_shift positive), then heads scaled against a0 = bn_shift: gate logits reach +-130, kernel logits spread by 150
        w["fc_w"] = 1e-3 * w["fc_w"]
        w["bn_shift"] = g.uniform(0.5, 1.5, hidden)
        a0 = w["bn_shift"]
        for p in ("ch", "fl", "sp"):
            if p == "fl" and cout == 1:
                continue
            lg = w[p + "_w"] @ a0 + w[p + "_b"]
            f = 130.0 / np.abs(lg).max()
            w[p + "_w"], w[p + "_b"] = f * w[p + "_w"], f * w[p + "_b"]
        lg = w["kn_w"] @ a0 + w["kn_b"]
        if knum > 1:
            f = 150.0 / (lg.max() - lg.min())
            w["kn_w"], w["kn_b"] = f * w["kn_w"], f * w["kn_b"]
            w["kn_b"][int(np.argmax(lg))] += 40.0          # the runner-up is 40 below: one-hot to 4e-18
    elif name == "uniform_k":
        w["kn_w"], w["kn_b"] = np.zeros((knum, hidden)), np.zeros(knum)
        base = n(cin * 9, cout, cin, 3, 3)
        sign = (1.0 - 2.0 * (np.arange(knum) % 2)).reshape(-1, 1, 1, 1, 1)
        w["bank"] = sign * base[None] + 1e-4 * w["bank"]
    elif name == "decades":
        w["bank"] = w["bank"] * 10.0 ** g.uniform(-3, 3, (1, cout, 1, 1, 1)) * 10.0 ** g.uniform(-3, 3, (1, 1, cin, 1, 1))
    else:
        assert name == "synth", name
    return {k: _f(v) for k, v in w.items()}


def from_state_dict(sd, pfx: str) -> dict:
    """The same dict from an OSConv of a SAVSR state dict (the engine's folding of the eval-mode BatchNorm: packing._add_osconv)."""
    from savsr_amd.packing import BN_EPS
    a = pfx + ".attention"
    g = lambda k: sd[k].detach().reshape(sd[k].shape[0], -1).numpy() if sd[k].dim() > 1 else sd[k].detach().numpy()      # noqa: E731
    bn_s = sd[a + ".bn.weight"] / torch.sqrt(sd[a + ".bn.running_var"] + BN_EPS)
    bn_b = sd[a + ".bn.bias"] - sd[a + ".bn.running_mean"] * bn_s
    w = dict(l1_w=g(pfx + ".scale_routing.0.weight"), l1_b=g(pfx + ".scale_routing.0.bias"), l2_w=g(pfx + ".scale_routing.2.weight"),
             l2_b=g(pfx + ".scale_routing.2.bias"), fc_w=g(a + ".fc.weight"), bn_scale=bn_s.numpy(), bn_shift=bn_b.numpy(),
             ch_w=g(a + ".channel_fc.weight"), ch_b=g(a + ".channel_fc.bias"), fl_w=g(a + ".filter_fc.weight"), fl_b=g(a + ".filter_fc.bias"),
             sp_w=g(a + ".spatial_fc.weight"), sp_b=g(a + ".spatial_fc.bias"), kn_w=g(a + ".kernel_fc.weight"), kn_b=g(a + ".kernel_fc.bias"),
             bank=sd[pfx + ".weight"].detach().numpy())
    return {k: _f(v) for k, v in w.items()}


def geom_of(w: dict):
    knum, cout, cin = w["bank"].shape[:3]
    return cin, cout, w["fc_w"].shape[0], knum


# ----------------------------------------------------------------------------- partial-sum regimes
@lru_cache(maxsize=None)
def partials(regime: str, nblk: int, c: int) -> np.ndarray:
    """[nblk][c] fp32 block sums of regime `regime` (shared, read-only).  `integers` are positive and sum below 2^24; `mean50` is positive."""
    g = np.random.RandomState([REGIMES.index(regime), nblk, c])
    if regime == "gauss":
        p = 8.0 * g.standard_normal((nblk, c))
    elif regime == "mean50":
        p = 128.0 * (50.0 + g.standard_normal((nblk, c)))
    elif regime == "altsign":
        p = (1.0 - 2.0 * (np.arange(nblk) % 2))[:, None] * (10.0 + np.abs(g.standard_normal((nblk, c))))
    elif regime == "integers":
        p = g.randint(1, 1000, (nblk, c)).astype(np.float64)
    elif regime == "zero":
        p = np.zeros((nblk, c))
    elif regime == "lastblock":
        p = np.zeros((nblk, c))
        p[nblk - 1] = 3.0 + g.standard_normal(c)
    else:
        assert regime == "decades", regime
        p = g.standard_normal((nblk, c)) * 10.0 ** g.uniform(-3, 3, (1, c))
    p = _f(p)
    p.setflags(write=False)
    return p


def inv_n_of(nblk: int) -> np.float32:
    """1 / (pixels): 128 pixels per block."""
    return F32(1.0 / (128 * nblk))


# ----------------------------------------------------------------------------- fp32 restatements of the kernels' orders
def mean32(partial: np.ndarray, inv_n, parts: int) -> np.ndarray:
    nblk, c = partial.shape
    s = np.zeros((parts, c), dtype=F32)
    for b in range(nblk):
        s[b % parts] = s[b % parts] + partial[b]
    t = np.zeros(c, dtype=F32)
    for pt in range(parts):
        t = t + s[pt]
    return (t * F32(inv_n)).astype(F32)


def wave_dot32(w: np.ndarray, v: np.ndarray, skip_col=None) -> np.ndarray:
    """wave_dot per row of w [rows][n] on v [n] in fp32: per lane the chain over columns lane + 64 j (products rounded, no FMA), then the
    butterfly v += shfl_xor(v, o) for o = 32 .. 1; lane 0's value.  skip_col: that column is left out (a defect)."""
    rows, n = w.shape
    q = (n + 63) // 64
    wp = np.zeros((rows, 64 * q), dtype=F32)
    vp = np.zeros(64 * q, dtype=F32)
    wp[:, :n], vp[:n] = w, v
    if skip_col is not None:
        wp[:, skip_col] = 0
    acc = np.zeros((rows, 64), dtype=F32)
    for j in range(q):
        acc = acc + (wp[:, 64 * j:64 * j + 64] * vp[None, 64 * j:64 * j + 64]).astype(F32)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    assert acc.dtype == F32
    return acc[:, 0]


def sigmoid32(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return (F32(1) / (F32(1) + np.exp(-x.astype(F32)).astype(F32))).astype(F32)


def _d(a) -> np.ndarray:
    return np.asarray(a, dtype=np.float64)


def sigmoid64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))


# ----------------------------------------------------------------------------- float64 references, stage by stage
def mean_reference(partial: np.ndarray, inv_n, parts: int = OSC_PARTS) -> dict:
    nblk = partial.shape[0]
    p = _d(partial)
    s = np.abs(p).sum(0) * float(inv_n)
    return dict(exact=p.sum(0) * float(inv_n), S=s, bound=gamma((nblk + parts - 1) // parts + parts + 1) * s, f32=mean32(partial, inv_n, parts))


def l1_reference(w: dict, partial: np.ndarray, inv_sh, inv_sw, inv_n, defect=None) -> dict:
    """partial -> v1.  defect (in `f32` only): ("lastcol",): the last column of L1 missing; ("swap",): inv_sh and inv_sw swapped.  `moved`: by how
    much the defect moves each pre-activation."""
    m = mean_reference(partial, inv_n)
    cin = partial.shape[1]
    v0 = np.concatenate([[float(inv_sh), float(inv_sw)], m["exact"]])
    e0 = np.concatenate([[0.0, 0.0], m["bound"]])
    W, b = _d(w["l1_w"]), _d(w["l1_b"])
    pre = W @ v0 + b
    s = np.abs(W) @ np.abs(v0) + np.abs(b)
    q = (cin + 2 + 63) // 64
    bound = gamma(q + 8) * (np.abs(W) @ (np.abs(v0) + e0) + np.abs(b)) + np.abs(W) @ e0
    v32 = np.concatenate([[F32(inv_sh), F32(inv_sw)], m["f32"]]).astype(F32)
    out = dict(exact=np.maximum(pre, 0), pre=pre, S=s, bound=bound, mean=m)
    if defect is not None and defect[0] == "swap":
        v32[[0, 1]] = v32[[1, 0]]
        out["moved"] = np.abs((W[:, 0] - W[:, 1]) * (v0[0] - v0[1]))
    skip = None
    if defect is not None and defect[0] == "lastcol":
        skip = cin + 1
        out["moved"] = np.abs(W[:, -1] * v0[-1])
    out["f32"] = np.maximum((wave_dot32(w["l1_w"], v32, skip) + w["l1_b"]).astype(F32), F32(0))
    if "moved" in out:      # a pre-activation that stays below zero on both sides does not show the defect
        pre_d = pre - (W[:, -1] * v0[-1] if skip is not None else (W[:, 0] - W[:, 1]) * (v0[0] - v0[1]))
        out["moved"] = np.abs(np.maximum(pre, 0) - np.maximum(pre_d, 0))
    return out


def l2_reference(w: dict, v1: np.ndarray) -> dict:
    """v1 (fp32, as the launch wrote it) -> v2."""
    W, b, v = _d(w["l2_w"]), _d(w["l2_b"]), _d(v1)
    s = np.abs(W) @ np.abs(v) + np.abs(b)
    q = (len(v) + 63) // 64
    return dict(exact=np.maximum(W @ v + b, 0), S=s, bound=gamma(q + 8) * s,
                f32=np.maximum((wave_dot32(w["l2_w"], _f(v1)) + w["l2_b"]).astype(F32), F32(0)))


def att_reference(w: dict, v2: np.ndarray) -> dict:
    """v2 (fp32, as the launch wrote it) -> att = ca [cin] | fa [cout] | sa [9] | ka [knum]: `exact`, `bound`, `S` (the logits' magnitude sums),
    `logit`, `e_l`, `f32`; `sig` = number of sigmoid entries."""
    cin, cout, hidden, knum = geom_of(w)
    v = _d(v2)
    fc, s_, t_ = _d(w["fc_w"]), _d(w["bn_scale"]), _d(w["bn_shift"])
    a = np.maximum((fc @ v) * s_ + t_, 0)
    s_a = np.abs(s_) * (np.abs(fc) @ np.abs(v)) + np.abs(t_)
    e_a = gamma((cin + 63) // 64 + 9) * s_a
    G = np.concatenate([_d(w[k]) for k in ("ch_w", "fl_w", "sp_w", "kn_w")])
    gb = np.concatenate([_d(w[k]) for k in ("ch_b", "fl_b", "sp_b", "kn_b")])
    logit = G @ a + gb
    s_l = np.abs(G) @ a + np.abs(gb)
    e_l = gamma(hidden + 1) * (np.abs(G) @ (a + e_a) + np.abs(gb)) + np.abs(G) @ e_a
    nsig = cin + cout + 9
    exact, bound = np.empty_like(logit), np.empty_like(logit)
    exact[:nsig] = sigmoid64(logit[:nsig])
    bound[:nsig] = e_l[:nsig] / 4 + 3 * U24
    lk, ek = logit[nsig:], e_l[nsig:]
    p = np.exp(lk - lk.max())
    ka = p / p.sum()
    delta = ek + U24 * ((lk.max() - lk) + 2 * ek.max())
    theta = np.exp(delta) * (1 + 2 * U24) - 1
    rel = (1 + theta) * (1 + U24) / ((1 - theta.max()) * (1 - gamma(knum))) - 1
    exact[nsig:], bound[nsig:] = ka, rel * ka + FLOOR
    # the fp32 restatement
    a32 = np.maximum(((wave_dot32(w["fc_w"], _f(v2)) * w["bn_scale"]).astype(F32) + w["bn_shift"]).astype(F32), F32(0))
    G32, acc = _f(G), np.zeros(len(gb), dtype=F32)
    for k in range(hidden):
        acc = acc + (G32[:, k] * a32[k]).astype(F32)
    acc = (acc + _f(gb)).astype(F32)
    f32 = np.empty(len(gb), dtype=F32)
    f32[:nsig] = sigmoid32(acc[:nsig])
    l32 = acc[nsig:]
    p32 = np.exp((l32 - l32.max()).astype(F32)).astype(F32)
    ssum = F32(0)
    for k in range(knum):
        ssum = F32(ssum + p32[k])
    f32[nsig:] = (p32 / ssum).astype(F32)
    return dict(exact=exact, bound=bound, S=s_l, logit=logit, e_l=e_l, f32=f32, sig=nsig, a=a)


def split_att(att: np.ndarray, geom):
    cin, cout, _, knum = geom
    return att[:cin], att[cin:cin + cout], att[cin + cout:cin + cout + 9], att[cin + cout + 9:]


def _decode32(x: np.ndarray, lo_mask=None) -> np.ndarray:
    """hi + lo of the split of fp32 x as float64; where lo_mask, the lo half is lost."""
    hi, lo = R.split(torch.from_numpy(np.ascontiguousarray(x, dtype=F32)))
    hi, lo = hi.double().numpy(), lo.double().numpy()
    if lo_mask is not None:
        lo = np.where(lo_mask, 0.0, lo)
    return hi + lo


def wy_transform(g: np.ndarray) -> np.ndarray:
    """[cout][cin][3 ky][3 kx] -> [4 pos][cout][cin][3 kx] in g's dtype, the kernel's order of operations."""
    half = g.dtype.type(0.5)
    sgl = g[:, :, 0] + g[:, :, 2]
    return np.stack([g[:, :, 0], half * (sgl + g[:, :, 1]), half * (sgl - g[:, :, 1]), g[:, :, 2]], 0)


def image_reference(w: dict, att: np.ndarray, wy: bool = False, defect=None, restate: bool = True) -> dict:
    """att (fp32, as the launch wrote it) -> the weight image's entries, [cout][cin][3 ky][3 kx] in the direct order (the order of
    conv_pack_index) or [4 pos][cout][cin][3 kx] in the Winograd-y order (conv_wy_pack_index): `exact`, `T`, `bound`, and `f32`: the fp32
    restatement decoded from its (hi, lo) split.
    defect (in `f32` only, direct order): ("lo", chunk, tap): the lo half of output channels 0 .. 31 x input chunk x tap lost; ("bank", k): bank k
    missing; ("sa_t",): the spatial gate indexed as (kx, ky).  `moved` is then what the defect moves per entry."""
    geom = geom_of(w)
    cin, cout, _, knum = geom
    ca, fa, sa, ka = (_d(x) for x in split_att(att, geom))
    bank = _d(w["bank"])
    kk = ka.reshape(-1, 1, 1, 1, 1)
    agg, mag = (kk * bank).sum(0), (kk * np.abs(bank)).sum(0)
    gate = fa[:, None, None, None] * sa.reshape(1, 1, 3, 3) * ca[None, :, None, None]
    g, t = agg * gate, mag * gate
    arith = gamma(knum + 3) * t
    out = {}
    if wy:
        out["exact"] = wy_transform(g)
        sb, sg = arith.sum(2), np.abs(g).sum(2)
        mid = 0.5 * ((1 + gamma(2)) * sb + gamma(2) * sg)
        a_ = np.stack([arith[:, :, 0], mid, mid, arith[:, :, 2]], 0)
        out["T"] = np.stack([t[:, :, 0], 0.5 * t.sum(2), 0.5 * t.sum(2), t[:, :, 2]], 0)
    else:
        out["exact"], a_, out["T"] = g, arith, t
    out["bound"] = a_ * (1 + SPLIT) + SPLIT * np.abs(out["exact"]) + FLOOR
    if not restate:
        return out
    ca32, fa32, sa32, ka32 = (_f(x) for x in split_att(att, geom))
    sa33 = sa32.reshape(3, 3)
    lo_mask = None
    if defect is not None and defect[0] == "sa_t":
        out["moved"] = np.abs(agg * fa[:, None, None, None] * ca[None, :, None, None] * (sa.reshape(3, 3) - sa.reshape(3, 3).T)[None, None])
        sa33 = sa33.T
    s = np.zeros(bank.shape[1:], dtype=F32)
    for k in range(knum):
        if defect is not None and defect[0] == "bank" and defect[1] == k:
            out["moved"] = np.abs(ka[k] * bank[k] * gate)
            continue
        s = s + (ka32[k] * w["bank"][k]).astype(F32)
    gco = (fa32[:, None, None, None] * sa33[None, None]).astype(F32)
    x = (s * (gco * ca32[None, :, None, None]).astype(F32)).astype(F32)
    if wy:
        x = wy_transform(x)
        assert x.dtype == F32
    elif defect is not None and defect[0] == "lo":
        _, chunk, tap = defect
        lo_mask = np.zeros(x.shape, dtype=bool)
        lo_mask[:32, 16 * chunk:16 * chunk + 16, tap // 3, tap % 3] = True
        hi = R.split(torch.from_numpy(x))[0].double().numpy()
        out["moved"] = np.where(lo_mask, np.abs(_decode32(x) - hi), 0.0)
    out["f32"] = _decode32(x, lo_mask)
    return out


# ----------------------------------------------------------------------------- SE gate and channel sums
@lru_cache(maxsize=None)
def se_weights(c: int, cmid: int) -> dict:
    g = np.random.RandomState([c, cmid])
    return dict(w1=_f(g.standard_normal((cmid, c)) / np.sqrt(c)), b1=_f(0.3 * g.standard_normal(cmid)),
                w2=_f(g.standard_normal((c, cmid))), b2=_f(0.5 * g.standard_normal(c)))


def se_reference(w: dict, partial: np.ndarray, inv_n) -> dict:
    """partial [nblk][c] -> the gate [c]: `exact`, `bound`, `f32`."""
    cmid, c = w["w1"].shape
    m = mean_reference(partial, inv_n, SE_PARTS)
    w1, b1, w2, b2 = (_d(w[k]) for k in ("w1", "b1", "w2", "b2"))
    z = np.maximum(w1 @ m["exact"] + b1, 0)
    e_z = gamma((c + 63) // 64 + 8) * (np.abs(w1) @ (np.abs(m["exact"]) + m["bound"]) + np.abs(b1)) + np.abs(w1) @ m["bound"]
    logit = w2 @ z + b2
    e_l = gamma(cmid + 1) * (np.abs(w2) @ (z + e_z) + np.abs(b2)) + np.abs(w2) @ e_z
    z32 = np.maximum((wave_dot32(w["w1"], m["f32"]) + w["b1"]).astype(F32), F32(0))
    acc = w["b2"].astype(F32)
    for k in range(cmid):
        acc = acc + (w["w2"][:, k] * z32[k]).astype(F32)
    return dict(exact=sigmoid64(logit), bound=e_l / 4 + 3 * U24, f32=sigmoid32(acc), S=np.abs(w2) @ z + np.abs(b2))


def sums_reference(x: np.ndarray, nblk: int) -> dict:
    """x [npx][ctot] fp32 (the sources side by side, src_ch channels each) -> partial [nblk][ctot]: `exact`, `S`, and `depth(src_ch)` for the bound
    gamma(depth) S.  Trailing blocks without pixels are zero."""
    npx, ctot = x.shape
    per = (npx + nblk - 1) // nblk
    exact, s = np.zeros((nblk, ctot)), np.zeros((nblk, ctot))
    for b in range(nblk):
        blk = _d(x[b * per:min(npx, b * per + per)])
        exact[b], s[b] = blk.sum(0), np.abs(blk).sum(0)
    return dict(exact=exact, S=s, per=per, depth=lambda src_ch: (per + (1024 // src_ch) - 1) // (1024 // src_ch) + 1024 // src_ch)


def worst(err: np.ndarray, bound: np.ndarray) -> float:
    """max over the elements with bound > 0 of err / bound (0 if there are none)."""
    msk = bound > 0
    return float((err[msk] / bound[msk]).max()) if bool(msk.any()) else 0.0
