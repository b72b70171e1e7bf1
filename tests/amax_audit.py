"""The amax invariant at every consumer: whenever hipnn hands out a word for a tensor, the word bounds that tensor.

``audit(monkeypatch)`` is a context manager for test modules.  It wraps ``hipnn.functional.amax_word_of`` -- every caller reaches it
as a module attribute, hipnn/fused.py and the models included --, and ``measured_amax_word`` (whose freshly measured word goes
straight to its consumer), and, whenever either returns a word for a tensor t, enqueues

    max|t| <= max(word) * (1 + slack)

on t's device, together with the calling function and t's shape.  On exit it synchronises ONCE and holds every result: violations
(``Audit.violations``), the rules whose words were asked for (``Audit.rules``), the largest bound-to-maximum ratio
(``Audit.max_ratio``; printed by the tests, never asserted: pooling and interpolation can make it arbitrarily large).  Nothing is
checked while a HIP graph is being captured (the audit runs eagerly only).

Which rule made a word is learnt by wrapping ``tag_amax`` as well (every rule tags through it) and looking at the calling frame:

    produced:<function>   a launch's own output bound (sstem_conv.h: the largest value it stored)                 slack 0
    measured              sstem_amax_f32 over the tensor                                                           slack 0
    hand_on:<caller>      hand_on_amax: pooling, its backward, the copy in _check, the alias of out=             the source's
    hand_on:upsample      hand_on_amax behind bilinear x2 up-sampling                                              the source's + N_UP_AMAX
    concat / sum / x16    tag_concat_amax, tag_sum_amax, the up-sampling backward                                  the largest of the parts'
                          (a sum of parts with slack n rounds once more: n + 1)
    concat_upsample       skip_cat_upsample2x (the up-sampled half stored straight into the concatenation)         as up-sampling

slack = n * 2^-24 with n counted per tensor.  N_UP_AMAX: the bilinear kernels compute lerp2(w0, a, w1, b) = fma(w1, b, rn(w0 a)) with
w0 = rn(1 - w1) (csrc/misc_kernels.hip).  With |a|, |b| <= M:  w0 <= (1 - w1)(1 + u),  rn(w0 a) <= w0 M (1 + u),  the fma rounds once
more:  |lerp2| <= (w1 M + (1 - w1) M (1 + u)^2)(1 + u) <= M (1 + u)^3, u = 2^-24.  The horizontal lerp2 feeds the vertical one:
M (1 + u)^6 <= M (1 + 7 u).  **N_UP_AMAX = 7**, counted as tests/stream_ref64.py counts its bounds (m rounded up to the next integer for
the second-order terms); tests/test_amax_audit_cpu.py searches heights and widths 1 .. 64 for the worst excess and holds it to this n."""
import contextlib
import sys

import torch

import hipnn.functional as HF

U = 2.0 ** -24
N_UP_AMAX = 7


class Audit(object):
    def __init__(self):
        self.records = []          # (caller, shape, rule, n) per check, in order
        self._viol = []            # 0-d bool tensors, one per check
        self._ratio = []           # 0-d float64 tensors: bound / maximum (inf for an all-zero tensor)
        self.skipped_in_capture = 0
        self.violations = None     # after exit: [(caller, shape, rule, n, ratio)]
        self.max_ratio = None
        self.rules = None          # after exit: {rule: number of words asked for}

    def __len__(self):
        return len(self.records)

    def _close(self):
        self.rules = {}
        for _, _, rule, _ in self.records:
            self.rules[rule] = self.rules.get(rule, 0) + 1
        if not self.records:
            self.violations, self.max_ratio = [], 0.0
            return
        for dev in {v.device for v in self._viol}:
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
        viol = [bool(v) for v in torch.stack([v.cpu() for v in self._viol]).tolist()]
        ratio = torch.stack([r.cpu() for r in self._ratio]).tolist()
        self.violations = [rec + (q,) for rec, bad, q in zip(self.records, viol, ratio) if bad]
        finite = [q for q in ratio if q != float("inf") and q == q]
        self.max_ratio = max(finite) if finite else 0.0

    def report(self):
        lines = ["%d words audited, %d violations, largest bound / maximum %.4g; rules: %s" % (
            len(self.records), len(self.violations), self.max_ratio, ", ".join("%s x%d" % kv for kv in sorted(self.rules.items())))]
        for caller, shape, rule, n, q in self.violations:
            lines.append("  VIOLATION in %s: tensor %s, word from rule %s (slack %d x 2^-24): bound / maximum = %.9g" % (caller, tuple(shape), rule, n, q))
        return "\n".join(lines)

    def assert_clean(self):
        assert not self.violations, self.report()


def _prov(t):
    p = getattr(t, "_amax_audit_rule", None)
    if p is None and getattr(t, "_base", None) is not None:
        p = getattr(t._base, "_amax_audit_rule", None)
    return p if p is not None else ("untracked", 0)


def _n_of(*ts):
    return max([_prov(t)[1] for t in ts if t is not None] or [0])


def _more(n, add):
    """(1 + n u)(1 + add u) <= 1 + (n + add + 1) u for the counts that occur (second-order terms: one unit)."""
    return n + add + (1 if n and add else 0)


_HELPERS = ("amax_word_of", "hand_on_amax", "tag_concat_amax", "tag_sum_amax", "measured_amax_word", "wrapped_word_of", "wrapped_tag", "wrapped_measured", "check")


def _outer_caller(frame):
    while frame is not None and frame.f_code.co_name in _HELPERS:
        frame = frame.f_back
    return frame.f_code.co_name if frame is not None else "?"


@contextlib.contextmanager
def audit(monkeypatch, up_slack=N_UP_AMAX):
    """with audit(monkeypatch) as a: ...   -- then a.assert_clean(), a.rules, a.max_ratio.  up_slack: the n of a word handed through
    bilinear up-sampling (the CPU mutants pass 0 to show that the count is needed)."""
    a = Audit()
    real_word_of, real_tag, real_measured = HF.amax_word_of, HF.tag_amax, HF.measured_amax_word
    code = {
        "hand_on": HF.hand_on_amax.__code__, "concat": HF.tag_concat_amax.__code__, "sum": HF.tag_sum_amax.__code__,
        "measured": HF.measured_amax_word.__code__, "x16": HF._UpsampleBilinear2x.backward.__code__,
        "concat_upsample": HF.skip_cat_upsample2x.__code__, "upsample": HF.upsample_bilinear2x_module.__code__,
    }

    def wrapped_tag(t, word):
        f = sys._getframe(1)
        c, loc = f.f_code, f.f_locals
        if c is code["hand_on"]:
            outer = f.f_back.f_code if f.f_back is not None else None
            if outer is code["upsample"]:
                rule, n = "hand_on:upsample", _more(_n_of(loc["src"]), up_slack)
            else:
                rule, n = "hand_on:" + _outer_caller(f.f_back), _n_of(loc["src"])
        elif c is code["concat"]:
            rule, n = "concat", _n_of(*loc["parts"])
        elif c is code["sum"]:
            k = _n_of(loc["a"], loc["b"])
            rule, n = "sum", (k + 1 if k else 0)                 # (parts that carry slack: the sum's own rounding on top)
        elif c is code["measured"]:
            rule, n = "measured", 0
        elif c is code["x16"]:
            rule, n = "x16", _n_of(loc["g"])
        elif c is code["concat_upsample"]:
            rule, n = "concat_upsample", max(_n_of(loc["skip"]), _more(_n_of(loc["x"]), up_slack))
        else:
            rule, n = "produced:" + c.co_name, 0
        r = real_tag(t, word)
        t._amax_audit_rule = (rule, n)
        return r

    def wrapped_word_of(t):
        w = real_word_of(t)
        if w is not None:
            check(t, w)
        return w

    def wrapped_measured(x):
        """A word measured HERE goes to the consumer without passing amax_word_of again: it is audited where it is made."""
        had = real_word_of(x) is not None
        w = real_measured(x)                                     # (asks the wrapped amax_word_of first: a word x already has is audited there)
        if not had:
            check(x, w)
        return w

    def check(t, w):
        if t.numel() == 0:
            return
        if t.is_cuda and torch.cuda.is_current_stream_capturing():
            a.skipped_in_capture += 1
            return
        rule, n = _prov(t)
        with torch.no_grad():
            m = t.detach().abs().max().double()
            b = w.detach().max().double()
            a._viol.append(~(m <= b * (1.0 + n * U)))
            a._ratio.append(b / m)
        a.records.append((_outer_caller(sys._getframe(2)), tuple(t.shape), rule, n))

    monkeypatch.setattr(HF, "tag_amax", wrapped_tag)
    monkeypatch.setattr(HF, "amax_word_of", wrapped_word_of)
    monkeypatch.setattr(HF, "measured_amax_word", wrapped_measured)
    try:
        yield a
    finally:
        monkeypatch.setattr(HF, "tag_amax", real_tag)
        monkeypatch.setattr(HF, "amax_word_of", real_word_of)
        monkeypatch.setattr(HF, "measured_amax_word", real_measured)
        a._close()
