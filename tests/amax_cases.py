"""Shared pieces of the amax tests (tests/test_amax_planted_gpu.py): where a maximum is planted, how a word is judged, words made by hand.

An amax word (include/sstem_conv.h) is 1024 float slots whose largest bounds a tensor.  The planted tests put ONE element of known
magnitude into an otherwise zero tensor, at the places a reduction can leave out, and demand of the word that comes back

    max(word) == |V stored|   exactly, and   every slot is 0 or |V stored|

-- a producer that misses the element leaves the word at zero; one that reads outside its tensor (guard bands hold 3e38) or reduces
something else than the stored values leaves a third value in some slot.  Nothing here needs a device to import."""
import torch

SLOTS = 1024
GUARD = 3.0e38                         # what the guard bands hold: any read outside the tensor shows in the word
SWEEP_SLOTS = (0, 3, 4, 255, 256, 511, 1023)    # the first / last lane and load of amax_word_max (64 lanes x four 16-byte loads)


def tile_of(T):
    """(tile width, tile height) of a split-kernel instance with tile parameter T (tests/test_conv_exact_gpu.py Inst.T)."""
    return (16, 16) if T == 16 else (32, 8)


def plant_positions(N, C, H, W, tw, th, cblock):
    """[(name, (n, c, y, x))]: the output elements a reduction can leave out for an [N, C, H, W] tensor produced in tw x th tiles,
    cblock channels per workgroup: the four plane corners, the last pixel of the last image in the last channel, a pixel inside the
    ragged right / bottom tile (the last column / row where the tiling is not ragged), the first pixel of the second tile, the last
    channel of a ragged channel block (the last channel otherwise).  Duplicates are dropped."""
    out, seen = [], set()

    def add(name, p):
        if p not in seen:
            seen.add(p)
            out.append((name, p))
    add("corner00", (0, 0, 0, 0)); add("corner0W", (0, 0, 0, W - 1)); add("cornerH0", (0, 0, H - 1, 0)); add("cornerHW", (0, 0, H - 1, W - 1))
    add("last", (N - 1, C - 1, H - 1, W - 1))
    xr = (W // tw) * tw + (W % tw) // 2 if W % tw else W - 1
    yb = (H // th) * th + (H % th) // 2 if H % th else H - 1
    add("ragged_right", (N - 1, min(1, C - 1), H // 2, xr))
    add("ragged_bottom", (0, min(2, C - 1), yb, W // 2))
    if W > tw:
        add("second_tile", (0, 0, 0, tw))
    elif H > th:
        add("second_tile", (0, 0, th, 0))
    add("last_channel", (0, C - 1, 0, 0))
    if C > cblock:
        add("second_block", (0, cblock, H // 2, W // 2))
    return out


def word_report(word, want):
    """None when the word says `want` (max == want, every slot 0 or want), else what is wrong with it."""
    w = word.detach().float().cpu().reshape(-1)
    assert w.numel() == SLOTS
    want = float(want)
    bad = torch.nonzero(~((w == 0) | (w == want))).reshape(-1)
    if bad.numel():
        return "%d slots hold neither 0 nor %r; first: slot %d = %r" % (bad.numel(), want, int(bad[0]), float(w[bad[0]]))
    if float(w.max()) != want:
        return "max(word) = %r, want %r" % (float(w.max()), want)
    if bool((torch.signbit(w) & (w == 0)).any()):
        return "a slot holds -0.0"
    return None


def assert_word(word, want, what):
    r = word_report(word, want)
    assert r is None, "%s: %s" % (what, r)


def hand_word(bound, slot, device="cpu"):
    """A word made by hand: `bound` in one slot (an int) or in every slot ("all")."""
    w = torch.zeros(SLOTS, dtype=torch.float32, device=device)
    if slot == "all":
        w.fill_(bound)
    else:
        w[slot] = bound
    return w


def predecessor(v):
    """The float32 below a positive float32 v."""
    t = torch.tensor(float(v), dtype=torch.float32)
    return float((t.view(torch.int32) - 1).view(torch.float32))


def amax_exponent(bound):
    """csrc/conv_split_common.h amax_exponent, restated: the biased exponent of the bound, at least 16; non-finite: 141 (scale 1)."""
    e = (int(torch.tensor(float(bound), dtype=torch.float32).view(torch.int32)) >> 23) & 0xFF
    if e == 255:
        e = 141
    return max(e, 16)


def scale_log2(bound):
    """log2 of the power-of-two scale a consumer multiplies a tensor with this bound by: 141 - e."""
    return 141 - amax_exponent(bound)
