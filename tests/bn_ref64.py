"""Float64 reference of the train-mode BatchNorm2d (+ ReLU / LeakyReLU) of csrc/norm_kernels.hip and the bounds of its every-element
checks (test infrastructure only; torch, any device).

    bn_geometry(N, C, HW)                                  -> (chunk_len, pieces, chunks)     bn_chunk_len / geom restated
    kernel_chunks(x)                                       -> chunk table of the statistics launch (one entry per workgroup)
    partition_triplets(x, n_partials, seed)                -> (float32 triplets [C, P, 3], chunk table) of an arbitrary partition
    bn_stats_ref64(x, eps, momentum, rm, rv, table)        -> dict: mean, var, invstd, unbiased, running_*; S_* of each
    bn_apply_ref64(x, mean, invstd, w, b, act, slope)      -> (y, S)
    bn_backward_ref64(dy, x, y, mean, invstd, w, act, slope, T, prior_dw, prior_db)
                                                           -> dict: dx, dweight, dbias; S_* and n_* of each
    mask_fixture()                                         -> the inputs on which two spellings of the pre-activation disagree in sign

Every function restates the operation as plain float64 tensor code that shares nothing with the kernels and runs on whatever device its
inputs are on.  The float32 scalars of the contract (momentum, eps, slope, weight, bias, and for the apply and the backward the saved
statistics) are taken as the float32 numbers they are and used in float64 from there on.

The check is stream_ref64.assert_within_rounding:  |got - ref| <= n * 2^-24 * S + 2^-120  at every element, u = 2^-24, where S is the sum
of the magnitudes of the terms the result sums and n the number of rounded fp32 operations on the longest path of one term (Higham 3.1,
3.4: gamma_m S, in any order, fused or not; a contracted multiply-add drops a rounding and never adds one, so every count is taken for
the uncontracted form).  n is m + 1 for gamma_m / (m u) - 1 < 1e-4 and the reference's own error; where S is a COMPOSITE, a sum of terms
each already multiplied by its own count, n is **N_COMPOSITE = 1.01** (as stream_ref64's Adam parameter).  None is tuned.

T = chunk_len / 256 (4, 8, 16, 32 or 64) is the number of elements of a full chunk that one of the 256 threads of a workgroup sums.

Statistics (bn_fwd_partial_body, channel_moments, the head of bn_fwd_apply_body)
-------------------------------------------------------------------------------
Chunk i of a channel holds L_i values x_ij; its pivot p_i is its first value; d_ij = x_ij - p_i.  A_i = sum_j |d_ij|, Q_i = sum_j d_ij^2,
dm_i = sum_j d_ij / L_i, m_i = p_i + dm_i (the chunk's mean), M2_i = sum_j (x_ij - m_i)^2.  The kernel:

  s_i   v = fl(x - p) (1), then a thread's sum: scalar path at most T terms, T - 1 rounded sums (0 + v is exact); vector path
        (v.x + v.y) + (v.z + v.w) (2), the sum into s once per group of four (at most T / 4 groups) and at most one tail element (1):
        1 + 2 + T / 4 + 1 <= T + 1 for T >= 4.                                              |s_i - sum d| <= (T + 1) u A_i
  q_i   v enters squared (2), the product (1), then the sums as above: scalar 3 + T - 1, vector 3 + 2 + T / 4 + 1 <= T + 3.
                                                                                             |q_i - sum d^2| <= (T + 3) u Q_i
  the tree reduction of the 256 per-thread values and everything up to the stores is double: below 2^-45 of the same magnitudes.
  mean  fl32(p_i + s_i / L_i): the sum's error over L_i and the store's own rounding.       e_i = u ((T + 1) A_i / L_i + |m_i|)
  M2    fl32(q_i - s_i^2 / L_i), d(s^2 / L) = 2 (s / L) ds:              E_i = u ((T + 3) Q_i + 2 (T + 1) |dm_i| A_i + M2_i)
  count exact (L_i <= 16384).
  Triplets formed elsewhere in float64 and rounded to float32 (``partials``) carry the store's rounding only: e_i = u |m_i|, E_i = u M2_i.

channel_moments merges the float32 triplets in double (n = sum L_i, its own error below 2^-45):
  mean' = sum L_i m_i / n                             |mean' - mean| <= sum L_i e_i / n =: E_pre
  save_mean = fl32(mean')                             **E_mean = E_pre + u |mean|**   (the store of the result itself)
  M2' = sum M2_i + sum L_i (m_i - mean')^2.  With eps_i the error of m_i, eb their weighted mean and D_i = m_i - mean (sum L_i D_i = 0):
  sum L_i (D_i + eps_i - eb)^2 - sum L_i D_i^2 = 2 sum L_i D_i eps_i + sum L_i (eps_i - eb)^2, the last at most sum L_i eps_i^2.
  THE ROUNDING OF EACH CHUNK MEAN TO FLOAT32 ENTERS HERE: e_i holds u |m_i|, which is of the size of the data, not of |x - pivot|; it is
  multiplied by |D_i|, the distance between chunk means, so on a channel of 1000 + randn it is some tens of u of the variance where
  E[x^2] - E[x]^2 in fp32 would lose all of it.      **E_var = (sum E_i + 2 sum L_i |D_i| e_i + sum L_i e_i^2) / n**
  save_invstd = fl32(1 / sqrt(var' + eps)), f(v) = 1 / sqrt(v + eps) decreasing and convex, var' clamped at 0:
                                                      **E_invstd = f(max(var - E_var, 0)) - f(var) + u f(max(var - E_var, 0))**
  running_mean = fl(fl(fl(1 - m) r) + fl(m save_mean)): the term (1 - m) r passes the difference, the product and the sum (3), m save_mean
  the product and the sum (2), and save_mean carries E_mean:
                                                      **E_rm = u (3 |(1 - m) r| + 2 |m mean|) + |m| E_mean**
  running_var likewise with fl32(unbiased) (1 more), unbiased = var n / (n - 1) in double:
                                                      **E_rv = u (3 |(1 - m) r| + 3 |m unbiased|) + |m| E_var n / (n - 1)**
  Each E is returned as S = E / u and checked with N_COMPOSITE.  At momentum 0 and 1 the expressions are exact up to what they carry.

Apply (bn_fwd_apply_body), held against float64 from the kernel's OWN save_mean / save_invstd
--------------------------------------------------------------------------------------------
  sc = fl(invstd w) (1);  sf = fl(b - fl(mean sc));  pre = fl(fl(x sc) + sf);  S = |x sc| + |mean sc| + |b|
  x sc:     sc, the product, the sum                               3
  mean sc:  sc, the product, the difference in sf, the sum         4
  b:        the difference, the sum                                2            **N_APPLY = 5**
ReLU adds nothing.  Where the kernel's pre and the reference's differ in sign, |pre| + |pre64| = |pre - pre64|, so either output is within
the same distance.  LeakyReLU multiplies the negative side by the slope, one more rounding: **N_APPLY_LEAKY = 6** on S * max(1, |slope|).

Backward (bn_bwd_partial_body, channel_totals, bn_bwd_apply_body)
-----------------------------------------------------------------
dz = dy act'(.), the mask taken from the forward launch's STORED y (y > 0), as torch's ReLU / LeakyReLU backward takes it;
xh = (x - mean) invstd from the saved statistics.  The kernel: dz = fl(dy slope) on the negative side (1, LeakyReLU only),
xh = fl(fl(x - mean) invstd) (2), a thread sums at most T + 1 terms one by one (T rounded sums), the chunk's sums are stored as float32
(1), summed over the chunks in double, and
  dbias   = fl32(sum dz)          1 + T + 1 + 1 = T + 3 on sum |dz|                         **n = T + N_DBIAS_X,   N_DBIAS_X = 4**
  dweight = fl32(sum dz xh)       1 + 2 + 1 (the product) + T + 1 + 1 = T + 6 on sum |dz xh|  **n = T + N_DWEIGHT_X, N_DWEIGHT_X = 7**
  with accumulate the stored value is fl32(prior + fl32(sum)): one rounding of the result more, |prior + sum| / n added to S.
  dx = fl(k fl(fl(dz - m_dz) - fl(xh m_dzx))), k = fl(w invstd), m_dz = fl32(sum dz / cnt), m_dzx = fl32(sum dz xh / cnt),
  S = |k| (|dz| + |m_dz| + |xh| |m_dzx|):
  dz:        its own rounding, the two differences, the product with k, k            5
  m_dz:      its store, the two differences, the product with k, k                   5
  xh m_dzx:  xh (2), m_dzx's store, the product, the difference, the product, k      7            **N_DX = 8**
  plus what the two means carry from their sums before the store:
  **carried = |k| u ((T + 2) sum |dz| + |xh| (T + 5) sum |dz xh|) / cnt**, folded into S as carried / (N_DX u).
"""
import numpy as np
import torch

from stream_ref64 import U, assert_within_rounding, f32  # noqa: F401  (re-exported for the tests)

BN_THREADS = 256
BN_CHUNK = 16384
N_COMPOSITE = 1.01
N_SUM_X = 1                # (T + 1) u on a chunk's sum of x - pivot
N_SQ_X = 3                 # (T + 3) u on a chunk's sum of (x - pivot)^2
N_APPLY = 5
N_APPLY_LEAKY = 6
N_DBIAS_X = 4
N_DWEIGHT_X = 7
N_DX = 8
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2


# ---- launch geometry ----------------------------------------------------------------------------------------------------------------------

def bn_geometry(N, C, HW):
    """(chunk_len, pieces per plane, chunks per channel) of both directions' launches: the grid is chunks x C workgroups."""
    length = BN_CHUNK
    while length > 1024 and N * C * ((HW + length - 1) // length) < 1024:
        length >>= 1
    pieces = (HW + length - 1) // length
    return length, pieces, N * pieces


def threads_terms(chunk_len):
    """T: the elements of a full chunk that one thread sums."""
    return chunk_len // BN_THREADS


# ---- chunk tables -------------------------------------------------------------------------------------------------------------------------

def kernel_chunks(x):
    """The chunks of the statistics launch on x [N, C, HW]: a dict of float64 [C, chunks] tensors L, m, M2, A, Q, dm (module docstring)
    and T."""
    N, C, HW = x.shape
    chunk_len, pieces, chunks = bn_geometry(N, C, HW)
    pad = pieces * chunk_len - HW
    xp = torch.nn.functional.pad(x.to(torch.float64), (0, pad)).view(N, C, pieces, chunk_len)
    valid = (torch.arange(pieces * chunk_len, device=x.device) < HW).view(1, 1, pieces, chunk_len)
    L = valid.sum(-1).to(torch.float64).expand(N, C, pieces)
    d = (xp - xp[..., :1]) * valid
    A = d.abs().sum(-1)
    dm = d.sum(-1) / L
    Q = (d * d).sum(-1)
    M2 = (((d - dm[..., None]) * valid) ** 2).sum(-1)
    m = xp[..., 0] + dm
    del d, xp
    flat = lambda t: t.permute(1, 0, 2).reshape(C, chunks).contiguous()
    return {"L": flat(L), "m": flat(m), "M2": flat(M2), "A": flat(A), "Q": flat(Q), "dm": flat(dm), "T": threads_terms(chunk_len)}


def partition_triplets(x, n_partials, seed, empty_mean=1.0e3):
    """An arbitrary partition of each channel's N * HW values (in (n, hw) order) into n_partials consecutive runs of unequal length, some
    of them empty: cut points drawn per channel, with repetitions.  Returns (triplets, table): triplets float32 [C, n_partials, 3] =
    (count, mean, M2) formed in float64 and rounded; an empty run carries count 0, the finite mean ``empty_mean`` and M2 = 0.  ``table``
    is the chunk table of bn_stats_ref64 for them (T = None: only the store's rounding)."""
    N, C, HW = x.shape
    M = N * HW
    rng = np.random.default_rng(seed)
    cuts = rng.integers(0, M + 1, size=(C, max(n_partials - 1, 0)))
    if n_partials >= 3:
        cuts[:, 1::3] = cuts[:, 0:-1:3]                    # a third of the cut points twice: empty runs at any n_partials >= 3
    cuts = np.sort(cuts, axis=1)
    cuts = torch.from_numpy(cuts.astype(np.int64)).to(x.device)
    xc = x.to(torch.float64).permute(1, 0, 2).reshape(C, M)
    ids = torch.searchsorted(cuts, torch.arange(M, device=x.device).expand(C, M).contiguous(), right=True)          # run of each element
    zeros = torch.zeros(C, n_partials, dtype=torch.float64, device=x.device)
    L = zeros.scatter_add(1, ids, torch.ones_like(xc))
    s = zeros.scatter_add(1, ids, xc)
    m = torch.where(L > 0, s / L.clamp(min=1.0), torch.full_like(s, empty_mean))
    M2 = zeros.scatter_add(1, ids, (xc - m.gather(1, ids)) ** 2)
    assert float(L.sum(1).min()) == M == float(L.sum(1).max())
    trip = torch.stack([L, m, M2], dim=2).to(torch.float32).contiguous()
    table = {"L": L, "m": m, "M2": M2, "A": zeros, "Q": zeros, "dm": zeros, "T": None}
    return trip, table


# ---- statistics ---------------------------------------------------------------------------------------------------------------------------

def _col(v, C, device):
    """None, a float32 tensor [C] or a Python float as float64 [C]."""
    if v is None:
        return None
    if torch.is_tensor(v):
        return v.to(torch.float64)
    return torch.full((C,), f32(v), dtype=torch.float64, device=device)


def bn_stats_ref64(x, eps, momentum, running_mean, running_var, table):
    """Batch statistics of x [N, C, HW] float32 and the running updates, float64 [C]: mean, var (biased), invstd, unbiased,
    running_mean, running_var (None where not tracked), and S_mean, S_var, S_invstd, S_running_mean, S_running_var: the derived error
    bounds of save_mean, the variance inside the kernel, save_invstd and the two running statistics, each divided by 2^-24 (check them
    with N_COMPOSITE).  ``table`` is the chunk table the kernel merges (kernel_chunks or partition_triplets)."""
    N, C, HW = x.shape
    n = float(N * HW)
    eps, mom = f32(eps), f32(momentum)
    x64 = x.to(torch.float64)
    mean = x64.mean(dim=(0, 2))
    var = ((x64 - mean[None, :, None]) ** 2).mean(dim=(0, 2))
    del x64
    f = lambda v: 1.0 / torch.sqrt(v + eps)
    invstd = f(var)
    unbiased = var * (n / (n - 1.0)) if n > 1 else var
    L, m, M2, A, Q, dm, T = (table[k] for k in ("L", "m", "M2", "A", "Q", "dm", "T"))
    if T is None:
        e = U * m.abs()
        E = U * M2
    else:
        e = U * ((T + N_SUM_X) * A / L.clamp(min=1.0) + m.abs())
        E = U * ((T + N_SQ_X) * Q + 2.0 * (T + N_SUM_X) * dm.abs() * A + M2)
    E_mean = (L * e).sum(1) / n + U * mean.abs()
    D = (m - mean[:, None]).abs()
    E_var = (E + 2.0 * L * D * e + L * e * e).sum(1) / n
    low = f((var - N_COMPOSITE * E_var).clamp(min=0.0))
    E_invstd = (low - invstd) + U * low
    out = {"mean": mean, "var": var, "invstd": invstd, "unbiased": unbiased, "S_mean": E_mean / U, "S_var": E_var / U,
           "S_invstd": E_invstd / U, "running_mean": None, "running_var": None}
    if running_mean is not None:
        r = running_mean.to(torch.float64)
        out["running_mean"] = (1.0 - mom) * r + mom * mean
        out["S_running_mean"] = 3.0 * ((1.0 - mom) * r).abs() + 2.0 * (mom * mean).abs() + abs(mom) * E_mean / U
    if running_var is not None:
        r = running_var.to(torch.float64)
        out["running_var"] = (1.0 - mom) * r + mom * unbiased
        out["S_running_var"] = (3.0 * ((1.0 - mom) * r).abs() + 3.0 * (mom * unbiased).abs()
                                + abs(mom) * E_var * ((n / (n - 1.0)) if n > 1 else 1.0) / U)
    return out


# ---- apply --------------------------------------------------------------------------------------------------------------------------------

def _act64(pre, act, slope):
    if act == ACT_RELU:
        return pre.clamp(min=0.0)
    if act == ACT_LEAKY:
        return torch.where(pre > 0, pre, pre * f32(slope))
    return pre


def apply_count(act):
    return N_APPLY_LEAKY if act == ACT_LEAKY else N_APPLY


def bn_apply_ref64(x, mean, invstd, weight, bias, act, slope):
    """act((x - mean) invstd w + b) on x [N, C, HW] in float64 from the float32 statistics and parameters given (weight / bias None:
    1 / 0).  Returns (y, S) with S = |x sc| + |mean sc| + |b|, times max(1, |slope|) under LeakyReLU; check with apply_count(act)."""
    C = x.shape[1]
    w = torch.ones(C, dtype=torch.float64, device=x.device) if weight is None else weight.to(torch.float64)
    b = torch.zeros(C, dtype=torch.float64, device=x.device) if bias is None else bias.to(torch.float64)
    sc = (invstd.to(torch.float64) * w)[None, :, None]
    msc = mean.to(torch.float64)[None, :, None] * sc
    x64 = x.to(torch.float64)
    pre = x64 * sc + (b[None, :, None] - msc)
    S = (x64 * sc).abs() + msc.abs() + b.abs()[None, :, None]
    if act == ACT_LEAKY:
        S = S * max(1.0, abs(f32(slope)))
    return _act64(pre, act, slope), S


# ---- backward -----------------------------------------------------------------------------------------------------------------------------

def bn_backward_ref64(dy, x, y, mean, invstd, weight, act, slope, T, prior_dweight=None, prior_dbias=None):
    """The backward of the train-mode BatchNorm + activation on [N, C, HW] float32 tensors in float64, the activation mask taken from the
    forward's stored ``y`` (y > 0; not used for act none).  Returns a dict: dx, S_dx (check with N_DX; what the two means carry is folded
    in), dweight, S_dweight, n_dweight, dbias, S_dbias, n_dbias.  With ``prior_*`` the parameter gradients are prior + sum and their S
    holds the one further rounding."""
    N, C, HW = x.shape
    cnt = float(N * HW)
    w = torch.ones(C, dtype=torch.float64, device=x.device) if weight is None else weight.to(torch.float64)
    col = lambda t: t.to(torch.float64)[None, :, None]
    dz = dy.to(torch.float64)
    if act == ACT_RELU:
        dz = torch.where(y > 0, dz, torch.zeros_like(dz))
    elif act == ACT_LEAKY:
        dz = torch.where(y > 0, dz, dz * f32(slope))
    xh = (x.to(torch.float64) - col(mean)) * col(invstd)
    sdz, sdzx = dz.sum(dim=(0, 2)), (dz * xh).sum(dim=(0, 2))
    Sdz, Sdzx = dz.abs().sum(dim=(0, 2)), (dz * xh).abs().sum(dim=(0, 2))
    n_db, n_dw = T + N_DBIAS_X, T + N_DWEIGHT_X
    out = {"dbias": sdz, "S_dbias": Sdz, "n_dbias": n_db, "dweight": sdzx, "S_dweight": Sdzx, "n_dweight": n_dw}
    if prior_dbias is not None:
        out["dbias"] = prior_dbias.to(torch.float64) + sdz
        out["S_dbias"] = Sdz + out["dbias"].abs() / n_db
    if prior_dweight is not None:
        out["dweight"] = prior_dweight.to(torch.float64) + sdzx
        out["S_dweight"] = Sdzx + out["dweight"].abs() / n_dw
    k = (w * invstd.to(torch.float64))[None, :, None]
    m_dz, m_dzx = (sdz / cnt)[None, :, None], (sdzx / cnt)[None, :, None]
    out["dx"] = k * (dz - m_dz - xh * m_dzx)
    S = k.abs() * (dz.abs() + m_dz.abs() + xh.abs() * m_dzx.abs())
    carried = k.abs() * ((T + 2) * Sdz[None, :, None] + xh.abs() * (T + 5) * Sdzx[None, :, None]) / cnt          # in units of u
    out["S_dx"] = S + carried / N_DX
    return out


# ---- the checks, shared by the float32 twin (CPU) and the kernels (GPU) -------------------------------------------------------------------

# (N, C, HW) -> (chunk_len, pieces, chunks), computed by hand from bn_chunk_len's loop
SHAPES = [
    ((2, 3, 35), (1024, 1, 2)),               # one chunk of 35; planes 1, 3, 5 start off 16-byte alignment (scalar path), 0, 2, 4 have a 3-element tail
    ((2, 4, 1), (1024, 1, 2)),                # two values per channel, len / 4 == 0
    ((1, 2, 1025), (1024, 2, 2)),             # last chunk of ONE element: the triplet (1, x, 0); the second channel starts at 1025
    ((3, 5, 3079), (1024, 4, 12)),            # 4 pieces, the last of 7
    ((300, 2, 6), (1024, 1, 300)),            # 300 chunks per channel: the stride loops of channel_moments / channel_totals wrap
    ((2, 700, 5), (16384, 1, 2)),             # 1400 workgroups: the amax slots wrap at 1024; 1400 >= 1024 keeps chunk_len at 16384
    ((1, 256, 8191), (2048, 4, 4)),           # 256 * 4 = 1024 stops the ladder at 2048; last chunk 2047
    ((1, 512, 16389), (16384, 2, 2)),         # 512 * 2 = 1024: chunk_len 16384, two pieces, the last of 5
]
SMALL = 6                                     # the first six run on the CPU twin too

# per shape: the nullable arguments and flags of the C-ABI, so that each value appears at least once
CONFIGS = [
    dict(affine=True, running=True, nbt=True, momentum=0.1, pgrads=True, accumulate=0),
    dict(affine=False, running=False, nbt=False, momentum=0.1, pgrads=False, accumulate=0),
    dict(affine=True, running=True, nbt=True, momentum=1.0, pgrads=True, accumulate=1),
    dict(affine=True, running=True, nbt=False, momentum=0.0, pgrads=True, accumulate=0),
    dict(affine=True, running=False, nbt=True, momentum=0.1, pgrads=True, accumulate=1),
    dict(affine=True, running=True, nbt=True, momentum=0.1, pgrads=False, accumulate=0),
    dict(affine=True, running=True, nbt=True, momentum=0.1, pgrads=True, accumulate=0),
    dict(affine=False, running=True, nbt=False, momentum=0.1, pgrads=True, accumulate=1),
]
EPS = 1e-5
ACTS = [(ACT_NONE, 0.0), (ACT_RELU, 0.0), (ACT_LEAKY, 0.2)]


def case_inputs(shape, cfg, generator, device="cpu"):
    """x, dy [N, C, HW] and the per-channel tensors of a case, float32, from ``generator``: x normal with a mean and a scale per channel,
    weights in [0.5, 1.5) with alternating signs, prior gradients of the size of the sums."""
    N, C, HW = shape
    rn = lambda *s: torch.randn(*s, generator=generator, device=device)
    x = (rn(N, C, HW) * (0.5 + torch.rand(1, C, 1, generator=generator, device=device) * 2.0) + rn(1, C, 1)).contiguous()
    dy = rn(N, C, HW)
    sign = torch.where(torch.arange(C, device=device) % 3 == 2, -1.0, 1.0)
    inp = {"x": x, "dy": dy, "weight": None, "bias": None, "running_mean": None, "running_var": None, "prior_dweight": None, "prior_dbias": None}
    if cfg["affine"]:
        inp["weight"] = (torch.rand(C, generator=generator, device=device) + 0.5) * sign
        inp["bias"] = rn(C) * 0.3
    if cfg["running"]:
        inp["running_mean"] = rn(C) * 0.1
        inp["running_var"] = torch.rand(C, generator=generator, device=device) + 0.5
    if cfg["pgrads"] and cfg["accumulate"]:
        inp["prior_dweight"] = rn(C) * (N * HW) ** 0.5
        inp["prior_dbias"] = rn(C) * (N * HW) ** 0.5
    return inp


def conditioning_inputs(generator, device="cpu"):
    """[2, 3, 1100] (chunks of 1024 and 76): channel 0 is 1000 + randn, channel 1 constant, channel 2 has an outlier of 1000 as the
    first element -- the pivot -- of every chunk."""
    inp = case_inputs((2, 3, 1100), CONFIGS[0], generator, device)
    x = inp["x"]
    x[:, 0] = 1000.0 + torch.randn(2, 1100, generator=generator, device=device)
    x[:, 1] = -3.25
    x[:, 2, 0] = 1000.0
    x[:, 2, 1024] = 1000.0
    return inp


def check_forward(got, inp, momentum, eps, act, slope, table, what):
    """Every statistic and every element of y of a forward launch (``got``: y, save_mean, save_invstd, running_mean, running_var) within
    its derived bound; y against float64 from got's own statistics.  Returns {name: worst err / bound}."""
    st = bn_stats_ref64(inp["x"], eps, momentum, inp["running_mean"], inp["running_var"], table)
    worst = {}
    for name, ref, S in (("save_mean", "mean", "S_mean"), ("save_invstd", "invstd", "S_invstd"),
                         ("running_mean", "running_mean", "S_running_mean"), ("running_var", "running_var", "S_running_var")):
        if st[ref] is None:
            assert got.get(name) is None, name
            continue
        worst[name] = assert_within_rounding(got[name], st[ref], st[S], N_COMPOSITE, "%s: %s" % (what, name)) / N_COMPOSITE
    ref, S = bn_apply_ref64(inp["x"], got["save_mean"], got["save_invstd"], inp["weight"], inp["bias"], act, slope)
    n = apply_count(act)
    worst["y"] = assert_within_rounding(got["y"], ref, S, n, "%s: y" % what) / n
    return worst


def check_backward(got, inp, y, save_mean, save_invstd, act, slope, T, what):
    """dx at every element, dweight and dbias (None: not asked for) of a backward launch within their derived bounds, the mask taken from
    the forward launch's stored ``y``.  Returns {name: worst err / bound}."""
    ref = bn_backward_ref64(inp["dy"], inp["x"], y, save_mean, save_invstd, inp["weight"], act, slope, T,
                            inp["prior_dweight"], inp["prior_dbias"])
    worst = {"dx": assert_within_rounding(got["dx"], ref["dx"], ref["S_dx"], N_DX, "%s: dx" % what) / N_DX}
    for name in ("dweight", "dbias"):
        if got.get(name) is not None:
            n = ref["n_" + name]
            worst[name] = assert_within_rounding(got[name], ref[name], ref["S_" + name], n, "%s: %s" % (what, name)) / n
    return worst


# ---- the mask fixture ---------------------------------------------------------------------------------------------------------------------

MASK_SHAPE = (2, 8, 2048)
MASK_NUDGES = (0, 1, -1, 2, -2, 0, 1, -1)          # ulps added to the bias of channel c
MASK_SEED = 5


def mask_fixture(seed=MASK_SEED):
    """Inputs on which the sign of the pre-activation decides many elements at once: x [2, 8, 2048] on multiples of 1 / 8 (flat regions of
    uint8 sections give such repeated values), weights in [0.5, 1.5), a gradient, and per channel the grid value the bias is aimed at.
    Returns CPU tensors (x, weight, dy, target); ``mask_bias`` completes it from a launch's own saved statistics."""
    g = torch.Generator().manual_seed(seed)
    N, C, HW = MASK_SHAPE
    x = torch.round(torch.randn(N, C, HW, generator=g) * 2.0 * 8.0) / 8.0 + torch.arange(C).view(1, C, 1) * 0.375
    weight = torch.rand(C, generator=g) + 0.5
    dy = torch.randn(N, C, HW, generator=g)
    pick = torch.randint(0, N * HW, (C,), generator=g)
    target = x.permute(1, 0, 2).reshape(C, -1).gather(1, pick[:, None])[:, 0].clone()
    return x.contiguous(), weight, dy, target


def mask_bias(save_mean, save_invstd, weight, target):
    """b = float32(-(v - mean) invstd w) in float64 from the float32 statistics, nudged by MASK_NUDGES ulps: the pre-activation of every
    element holding the grid value v is within a few ulps of b of zero."""
    b = (-(target.to(torch.float64) - save_mean.to(torch.float64)) * save_invstd.to(torch.float64) * weight.to(torch.float64)).to(torch.float32)
    bits = b.cpu().numpy().view(np.int32).copy()
    nudges = np.array(MASK_NUDGES, np.int32)
    bits = np.where(bits >= 0, bits + nudges, bits - nudges).astype(np.int32)          # the sign-magnitude order of float32
    out = torch.from_numpy(bits.view(np.float32).copy()).to(b.device)
    assert torch.isfinite(out).all() and (out != 0).all()
    return out
