"""A Python-integer model of the Goldilocks arithmetic in latticeum_amd/csrc/gl.hpp.

Three things live here, shared by tests/test_gl_model.py (no GPU), tests/test_gl_host.py
(the host compile of gl.hpp) and tests/test_gpu_gl.py (the device compile, through
lf_dev_gl_probe):

* edge_values(): the directed u64 values at which the carry and borrow fix-ups of gl.hpp
  change their mind, canonical (< p) and any-u64;
* one transliteration per primitive, on Python ints with the same limb steps as the C.
  Each returns (value, flags): flags names every decision the evaluation took, qualified
  by the primitive that took it ("reduce128.carry"). A primitive that calls another one
  reports the callee's flags too, OR-ed over its call sites. A flag is only present when
  the evaluation reached the decision;
* the vector sets (vector_sets()) and the branch census over them (census()).

The reference for every value is ref(): plain % p on Python integers. It is never one of
the transliterations; those exist to say which branches a vector takes.
"""
from __future__ import annotations

import functools
import random
from dataclasses import dataclass, field

P = (1 << 64) - (1 << 32) + 1
EPS = (1 << 32) - 1
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
R_INV = 0xFFFFFFFE00000001
CENSUS_MIN = 8

# op codes of lf_dev_gl_probe (latticeum_amd/csrc/gl_probe.hpp enum Op; test_gl_model.py
# checks the two lists agree)
OPS = {
    "canon": 0, "add": 1, "sub": 2, "neg": 3, "reduce128": 4, "mul": 5, "mul_pow2": 6, "mul_pow2_rt": 7,
    "shl96": 8, "shl192": 9, "shl_small_weak": 10, "add_weak": 11, "from_x_y32": 12, "acc_reduce": 13,
    "acc_add": 14, "cacc_reduce": 15, "cacc_reduce_weak": 16, "cacc_reduce_terms": 17, "fq3_mul": 18,
    "to_mont": 19, "from_mont": 20, "s_mul3": 21, "s_mul_w3": 22, "s_mad2_3": 23, "sacc3": 24, "fq3acc": 25,
}
# ops whose contract is "weakly reduced": any u64 congruent to the value
WEAK_OPS = ("reduce128", "shl_small_weak", "add_weak", "cacc_reduce_weak")
# ops that exist on the device only (slot.hpp, ring.hpp)
DEVICE_ONLY_OPS = ("s_mul3", "s_mul_w3", "s_mad2_3", "sacc3", "fq3acc")
# words per element
WORDS = {"fq3_mul": 3, "s_mul3": 3, "s_mul_w3": 3, "s_mad2_3": 3, "sacc3": 3, "fq3acc": 3}


# ------------------------------------------------------------------ the edge set
def edge_values():
    """(canonical, any_u64): deterministic, sorted, duplicate-free lists of u64"""
    v = {0, 1, 2, (1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1}
    for i in range(64):
        v |= {1 << i, (1 << i) - 1, P - (1 << i)}
    v |= {P - 1, P - 2, P - (1 << 32), P - (1 << 32) + 1}
    v |= {(P + 1) // 2, (P - 1) // 2, 1 << 63, (1 << 63) + 1, (1 << 63) - 1}
    v |= {0xFFFFFFFEFFFFFFFF, 0x00000001FFFFFFFF, 0xFFFF0000FFFF0000, 0x7FFFFFFF80000000}
    any64 = v | {P, P + 1, (1 << 64) - 2, (1 << 64) - 1} | EXTRA_ANY
    assert all(0 <= x <= M64 for x in any64)
    return sorted(x for x in v if x < P), sorted(any64)


# further values in [p, 2^64): the four above alone leave canon's fold short of CENSUS_MIN hits
EXTRA_ANY = {P + 2, P + (1 << 16), P + (1 << 31), (1 << 64) - (1 << 31), (1 << 64) - 3}


# ------------------------------------------------------------------ limb helpers
def _addc64(a, b):
    t = a + b
    return t & M64, t >> 64


def _subb64(a, b):
    t = a - b
    return t & M64, int(t < 0)


def _addc32(a, b, c):
    t = a + b + c
    return t & M32, t >> 32


def _subc32(a, b, c):
    t = a - b - c
    return t & M32, int(t < 0)


def _m(flags, sub):
    """a callee's flags into its caller's, OR-ed over the call sites (the joint one-hot flags,
    "x=..", mean nothing OR-ed: they stay with the primitive's own vector set)"""
    for k, v in sub.items():
        if "=" not in k:
            flags[k] = flags.get(k, False) or bool(v)


# ------------------------------------------------------------------ transliterations
def canon(x):
    u, c = _addc64(x, EPS)
    return (u if c else x), {"canon.ge_p": bool(c)}


def add(a, b):
    t, c1 = _addc64(a, b)
    u, c2 = _addc64(t, EPS)
    f = {"add.c1": bool(c1), "add.c2": bool(c2), "add.c1&c2": bool(c1 and c2), "add.sum_eq_p": a + b == P}
    return (u if (c1 | c2) else t), f


def sub(a, b):  # the device body: a 32-bit borrow chain
    dl, b1 = _subc32(a & M32, b & M32, 0)
    dh, b2 = _subc32(a >> 32, b >> 32, b1)
    d = (dh << 32) | dl
    f = {"sub.b1": bool(b1), "sub.borrow": bool(b2), "sub.eq": a == b}
    if b2:
        f["sub.fix_wrap"] = d < EPS
        d = (d - EPS) & M64
    return d, f


def neg(a):
    return (P - a if a else 0), {"neg.zero": a == 0}


def from_x_y32(X, Y):
    yh = Y >> 32
    U = (Y & M32) + yh
    c = U >> 32
    V = X - yh + c * EPS
    assert -(1 << 63) <= V < (1 << 63) and -(1 << 63) <= U < (1 << 63)
    t, carry = _addc64(V & M64, (U & M32) << 32)
    k = carry - int(V < 0)
    r = t + k * EPS
    f = {"from_x_y32.c=-1": c == -1, "from_x_y32.c=0": c == 0, "from_x_y32.c=1": c == 1,
         "from_x_y32.k=-1": k == -1, "from_x_y32.k=0": k == 0, "from_x_y32.k=1": k == 1,
         "from_x_y32.carry": bool(carry), "from_x_y32.V<0": V < 0, "from_x_y32.c_other": not -1 <= c <= 1,
         "from_x_y32.k_fix_wrap": not 0 <= r <= M64}
    v, g = canon(r & M64)
    _m(f, g)
    return v, f


def mul_wide(a, b):  # the device body: four 32 x 32 multiply-adds, no decision in it
    a0, a1, b0, b1 = a & M32, a >> 32, b & M32, b >> 32
    p0 = a0 * b0
    t = a0 * b1 + (p0 >> 32)
    u = a1 * b0 + (t & M32)
    hi = a1 * b1 + (t >> 32) + (u >> 32)
    lo = ((u << 32) & M64) | (p0 & M32)
    assert t <= M64 and u <= M64 and hi <= M64 and lo + (hi << 64) == a * b
    return lo, hi


def reduce128(lo, hi):
    h0, h1 = hi & EPS, hi >> 32
    r, c = _addc64(lo, h0 * EPS)
    f = {"reduce128.carry": bool(c)}
    if c:
        f["reduce128.carry_fix_wrap"] = r + EPS > M64
        r = (r + EPS) & M64
    s, b = _subb64(r, h1)
    f["reduce128.borrow"] = bool(b)
    if b:
        f["reduce128.borrow_fix_wrap"] = s < EPS
        s = (s - EPS) & M64
    for cc in (0, 1):
        for bb in (0, 1):
            f[f"reduce128.carry={cc},borrow={bb}"] = (c, b) == (cc, bb)
    f["reduce128.ge_p"] = s >= P
    return s, f


def mul(a, b):
    lo, hi = mul_wide(a, b)
    s, f = reduce128(lo, hi)
    v, g = canon(s)
    _m(f, g)
    return v, f


def mul_pow2(a, s, const_s=False):
    """const_s: the caller's s is a constant (fq3_mul's 40), so the decisions on s are none"""
    f = {}
    negate = s >= 96
    if negate:
        s -= 96
    if not const_s:
        f["mul_pow2.negate"] = negate
        f["mul_pow2.limb_split"] = s >= 64
    if s < 64:
        if not const_s:
            f["mul_pow2.s_zero"] = s == 0
        lo, hi = ((a << s) & M64, a >> (64 - s)) if s else (a, 0)
        w, g = reduce128(lo, hi)
        _m(f, g)
        r, g = canon(w)
        _m(f, g)
    else:
        t = s - 64
        if not const_s:
            f["mul_pow2.t_zero"] = t == 0
        lo, hi = ((a << t) & M64, a >> (64 - t)) if t else (a, 0)
        w, g = reduce128(0, lo)
        _m(f, g)
        x, g = canon(w)
        _m(f, g)
        y, g = canon(hi << 32)
        _m(f, g)
        r, g = sub(x, y)
        _m(f, g)
    if negate:
        r, g = neg(r)
        _m(f, g)
    return r, f


def shl96(x, s):
    x0, x1 = x & M32, x >> 32
    f = {"shl96.s_zero": s == 0, "shl96.form1": 0 < s < 32, "shl96.form2": 32 <= s < 64, "shl96.form3": s >= 64}
    if s == 0:
        return x, f
    if s < 32:
        lo = (x << s) & M64
        nq = (x >> (64 - s)) * EPS + EPS
        f["shl96.f1.nq_wrap"] = nq > M64
        tl, c1 = _addc32(lo & M32, nq & M32, 0)
        th, c2 = _addc32(lo >> 32, (nq >> 32) & M32, c1)
        t = (th << 32) | tl
        f["shl96.f1.c1"], f["shl96.f1.c2"] = bool(c1), bool(c2)
        return (t if c2 else (t + P) & M64), f
    if s < 64:
        u = s - 32
        f["shl96.f2.u_zero"] = u == 0
        y0 = (x0 << u) & M32 if u else x0
        y1 = (x >> (32 - u)) & M32 if u else x1
        y2 = x1 >> (32 - u) if u else 0
        al, c = _addc32(y0, y1, 0)
        ll, lh = _addc32(y1, y2, c)
        rl, b1 = _subc32(0, ll, 0)
        f["shl96.f2.h_wrap"] = al + c > M32
        rh, b2 = _subc32((al + c) & M32, lh, b1)
        f.update({"shl96.f2.c": bool(c), "shl96.f2.lh": bool(lh), "shl96.f2.b1": bool(b1), "shl96.f2.b2": bool(b2)})
        r, br = (rh << 32) | rl, b2
    else:
        k = 96 - s
        f["shl96.f3.k32"] = k == 32
        C = (x0 << (32 - k)) & M32
        m, a = C * EPS, x >> k
        rl, b1 = _subc32(m & M32, a & M32, 0)
        rh, b2 = _subc32(m >> 32, a >> 32, b1)
        f.update({"shl96.f3.b1": bool(b1), "shl96.f3.b2": bool(b2)})
        r, br = (rh << 32) | rl, b2
    return ((r + P) & M64 if br else r), f


def shl192(x, e):
    f = {"shl192.negate": e >= 96}
    v, g = shl96(x, e if e < 96 else e - 96)
    _m(f, g)
    if e >= 96:
        v, g = neg(v)
        _m(f, g)
    return v, f


def shl_small_weak(x, s):
    lo, hi = (x << s) & M64, x >> (64 - s)
    t, c = _addc64(lo, hi * EPS)
    f = {"shl_small_weak.c": bool(c)}
    if c:
        f["shl_small_weak.fix_wrap"] = t + EPS > M64
        t = (t + EPS) & M64
    return t, f


def add_weak(a, b):
    t, c = _addc64(a, b)
    f = {"add_weak.c": bool(c)}
    if c:
        f["add_weak.fix_wrap"] = t + EPS > M64
        t = (t + EPS) & M64
    return t, f


def to_mont(a):
    return mul(a, EPS)


def from_mont(m):
    c, f = canon(m)
    v, g = mul(c, R_INV)
    _m(f, g)
    return v, f


def fq3_mul(a, b):
    f = {}

    def call(fn, *args, **kw):
        v, g = fn(*args, **kw)
        _m(f, g)
        return v

    a0, a1, a2 = a
    b0, b1, b2 = b
    t0 = call(add, call(mul, a1, b2), call(mul, a2, b1))
    c0 = call(add, call(mul, a0, b0), call(mul_pow2, t0, 40, const_s=True))
    c1 = call(add, call(add, call(mul, a0, b1), call(mul, a1, b0)), call(mul_pow2, call(mul, a2, b2), 40, const_s=True))
    c2 = call(add, call(add, call(mul, a0, b2), call(mul, a1, b1)), call(mul, a2, b0))
    return (c0, c1, c2), f


# ---- Acc: (lo, hi, top)
def acc_mad(s, a, b):
    lo, hi, top = s
    plo, phi = mul_wide(a, b)
    nlo = (lo + plo) & M64
    c = int(nlo < plo)
    f = {"acc_mad.lo_carry": bool(c), "acc_mad.hi_wrap": phi + c > M64}
    phi = (phi + c) & M64
    nhi = (hi + phi) & M64
    t = int(nhi < phi)
    f["acc_mad.top_carry"] = bool(t)
    f["acc_mad.top_wrap"] = top + t > M32
    return (nlo, nhi, (top + t) & M32), f


def acc_add(s, v):
    lo, hi, top = s
    nlo = (lo + v) & M64
    c = int(nlo < v)
    nhi = (hi + c) & M64
    t = int(nhi < c)
    f = {"acc_add.lo_carry": bool(c), "acc_add.top_carry": bool(t), "acc_add.top_wrap": top + t > M32}
    return (nlo, nhi, (top + t) & M32), f


def acc_reduce(s):
    lo, hi, top = s
    f = {"acc_reduce.top_nz": top != 0}
    w, g = reduce128(lo, hi)
    _m(f, g)
    r, g = canon(w)
    _m(f, g)
    t, g = canon(top << 32)
    f["acc_reduce.top_ge_p"] = g["canon.ge_p"]
    v, g = sub(r, t)
    _m(f, g)
    return v, f


# ---- CAcc: (s0, s1, s2, c0, c1, c2)
def cacc_mad(a, x, y):
    s0, s1, s2, c0, c1, c2 = a
    x0, x1, y0, y1 = x & M32, x >> 32, y & M32, y >> 32
    s0, k0 = _addc64(s0, x0 * y0)
    s1, k1a = _addc64(s1, x0 * y1)
    s1, k1b = _addc64(s1, x1 * y0)
    s2, k2 = _addc64(s2, x1 * y1)
    f = {"cacc_mad.k0": bool(k0), "cacc_mad.k1a": bool(k1a), "cacc_mad.k1b": bool(k1b), "cacc_mad.k2": bool(k2),
         "cacc_mad.count_wrap": max(c0 + k0, c1 + k1a + k1b, c2 + k2) > M32}
    return (s0, s1, s2, (c0 + k0) & M32, (c1 + k1a + k1b) & M32, (c2 + k2) & M32), f


def cacc_reduce_weak(a):
    s0, s1, s2, c0, c1, c2 = a
    s0l, s0h, s1l, s1h, s2l, s2h = s0 & M32, s0 >> 32, s1 & M32, s1 >> 32, s2 & M32, s2 >> 32
    x1, k1 = _addc32(s0h, s1l, 0)
    y, ka = _addc32(s1h, s2l, k1)
    x2, kb = _addc32(y, c0, 0)
    z, kc = _addc32(s2h, c1, ka)
    x3, kd = _addc32(z, 0, kb)
    x4 = c2 + kc + kd
    f = {"cacc_reduce_weak." + n: bool(v) for n, v in (("k1", k1), ("ka", ka), ("kb", kb), ("kc", kc), ("kd", kd))}
    f["cacc_reduce_weak.kc&kd"] = bool(kc and kd)
    f["cacc_reduce_weak.x4_nz"] = x4 != 0
    f["cacc_reduce_weak.x4_wrap"] = x4 > M32
    x4 &= M32
    uh, c = _addc32(x1, x2, 0)
    ul, c2a = _addc32(s0l, (0 - c) & M32, 0)
    uh, c2b = _addc32(uh, 0, c2a)
    vh, b = _subc32(uh, x4, 0)
    vl, b2a = _subc32(ul, (0 - b) & M32, 0)
    vh, b2b = _subc32(vh, 0, b2a)
    sl, sc = _addc32(x2, x3, 0)
    wl, b3a = _subc32(vl, sl, 0)
    wh, b3 = _subc32(vh, sc, b3a)
    wl, b4a = _subc32(wl, (0 - b3) & M32, 0)
    wh, b4b = _subc32(wh, 0, b4a)
    for n, v in (("c", c), ("c2", c2a), ("u_second_carry", c2b), ("b", b), ("b2", b2a), ("v_second_borrow", b2b),
                 ("sc", sc), ("b3_lo", b3a), ("b3", b3), ("b4", b4a), ("w_second_borrow", b4b)):
        f["cacc_reduce_weak." + n] = bool(v)
    return (wh << 32) | wl, f


def cacc_reduce(a):
    w, f = cacc_reduce_weak(a)
    v, g = canon(w)
    _m(f, g)
    return v, f


def cacc_reduce_terms(a):
    s0, s1, s2, c0, c1, c2 = a
    f = {}

    def call(fn, *args):
        v, g = fn(*args)
        _m(f, g)
        return v

    r = call(canon, s0)
    r = call(add, r, call(canon, c0 * EPS))
    r = call(add, r, call(canon, ((s1 & EPS) << 32)))
    r = call(add, r, call(canon, (s1 >> 32) * EPS))
    r = call(sub, r, call(canon, c1))
    r = call(add, r, call(canon, call(reduce128, 0, s2)))
    r = call(sub, r, call(canon, c2 << 32))
    return r, f


def acc_value(s):
    return s[0] + (s[1] << 64) + (s[2] << 128)


def cacc_value(a):
    s0, s1, s2, c0, c1, c2 = a
    return s0 + (s1 << 32) + ((s2 + c0) << 64) + (c1 << 96) + (c2 << 128)


# flags that cannot be taken under the function's stated precondition, each with its proof.
# A key is (primitive, flag), or ("*", flag) where it holds for every caller in gl.hpp.
UNREACHABLE = {
    ("*", "add.c1&c2"): "canonical a, b: a + b <= 2p - 2, so after a carry t = a + b - 2^64 <= 2^64 - 2^33 and "
                        "t + EPS < 2^64",
    ("*", "sub.fix_wrap"): "after a borrow d = a - b + 2^64 >= 2^64 - (p - 1) = 2^32 > EPS",
    ("*", "reduce128.carry_fix_wrap"): "lo + h0 EPS <= 2^64 - 1 + (2^32 - 1)^2, so after a carry r <= 2^64 - 2^33 and "
                                       "r + EPS < 2^64",
    ("*", "reduce128.borrow_fix_wrap"): "after a borrow s = r - h1 + 2^64 > 2^64 - 2^32 > EPS",
    ("*", "reduce128.carry=1,borrow=1"): "after a carry r was raised by EPS, so r >= EPS >= h1: no borrow",
    ("mul_pow2", "sub.b1"): "the subtrahend canon(hi << 32) has a zero low word",
    ("mul_pow2_rt", "sub.b1"): "the subtrahend canon(hi << 32) has a zero low word",
    ("acc_reduce", "sub.b1"): "the subtrahend top << 32 has a zero low word",
    ("to_mont", "reduce128.borrow"): "a EPS < 2^96, so h1 = 0",
    ("to_mont", "reduce128.carry=0,borrow=1"): "a EPS < 2^96, so h1 = 0",
    ("from_mont", "reduce128.borrow"): "T = c EPS^2 (R_INV = EPS^2). A borrow needs h0 = 0 and lo < h1, so T = lo + "
                                       "2^96 h1; 2^96 == 1 mod EPS gives lo + h1 = EPS, and 2^96 == 3 EPS + 1 mod "
                                       "EPS^2 then gives EPS | 1 + 3 h1, impossible as 3 | EPS",
    ("cacc_reduce_terms", "reduce128.carry"): "its one call is reduce128(0, s2): 0 + h0 EPS < 2^64",
    ("cacc_reduce_terms", "reduce128.ge_p"): "reduce128(0, s2): without a borrow s <= (2^32 - 1)^2 < p; a borrow needs "
                                             "h0 = 0 and leaves s = p - h1 < p",
    ("*", "from_x_y32.c_other"): "U = yl + yh with 0 <= yl < 2^32 and -2^30 <= yh < 2^30, so U >> 32 is -1, 0 or 1",
    ("*", "from_x_y32.k_fix_wrap"): "the 65-bit sum V + ul 2^32 lies in (-2^63, 2^64 + 2^63): t < 2^63 when k = 1 "
                                    "and t > 2^63 when k = -1, so t + k EPS stays in [0, 2^64)",
    ("*", "shl96.f1.nq_wrap"): "x >> (64 - s) < 2^31, so nq = (hi + 1) EPS < 2^63",
    ("*", "shl96.f2.h_wrap"): "when y0 + y1 carries, al = y0 + y1 - 2^32 <= 2^32 - 2, so al + 1 < 2^32",
    ("*", "shl_small_weak.fix_wrap"): "after a carry t = lo + hi EPS - 2^64 < hi EPS < 2^63, so t + EPS < 2^64",
    ("*", "add_weak.fix_wrap"): "after a carry t = a + b - 2^64 < b < p, so t + EPS < 2^64",
    ("*", "acc_mad.hi_wrap"): "the high word of a 64 x 64 product is <= 2^64 - 2, so hi + 1 does not wrap",
    ("*", "acc_mad.top_wrap"): "top counts one carry per product: below 2^32 for fewer than 2^32 products",
    ("*", "acc_add.top_wrap"): "top counts one carry per call: below 2^32 for fewer than 2^32 calls",
    ("*", "acc_reduce.top_ge_p"): "top < 2^32, so top 2^32 <= 2^64 - 2^32 = p - 1",
    ("*", "cacc_mad.count_wrap"): "each counter grows by at most 2 per product: below 2^32 for fewer than 2^31 "
                                  "products",
    ("*", "cacc_reduce_weak.x4_wrap"): "c2 + kc + kd <= (number of products) + 2 < 2^32",
    ("*", "cacc_reduce_weak.kc&kd"): "kc leaves z = s2h + c1 + ka - 2^32 <= c1, a count below 2^32 - 1, so z + kb cannot carry",
    ("*", "cacc_reduce_weak.u_second_carry"): "with c, uh = x1 + x2 - 2^32 <= 2^32 - 2 and uh + c2 stays below 2^32; without c, c2 = 0",
    ("*", "cacc_reduce_weak.v_second_borrow"): "with b, vh = uh - x4 + 2^32 >= 2 (x4 is a count below 2^32 - 1) and absorbs b2; without b, b2 = 0",
    ("*", "cacc_reduce_weak.w_second_borrow"): "with b3, wh = vh - sc - b3_lo + 2^32 >= 2^32 - 2 and absorbs b4; without b3, b4 = 0",
}


def unreachable(prim, flag):
    return ("*", flag) in UNREACHABLE or (prim, flag) in UNREACHABLE


# ------------------------------------------------------------------ the mathematical reference
def fq3_ref(a, b):
    """Fq[u]/(u^3 - 2^40) on Python ints"""
    nr = 1 << 40
    a0, a1, a2 = a
    b0, b1, b2 = b
    return ((a0 * b0 + nr * (a1 * b2 + a2 * b1)) % P, (a0 * b1 + a1 * b0 + nr * a2 * b2) % P,
            (a0 * b2 + a1 * b1 + a2 * b0) % P)


def _s64(x):
    return x - (1 << 64) if x >> 63 else x


def ref(op, a, b, s, m):
    """the value of one case: a, b the case's operand words (m, or m x 3, of them)"""
    if op == "canon":
        return a[0] % P
    if op == "add":
        return (a[0] + b[0]) % P
    if op == "sub":
        return (a[0] - b[0]) % P
    if op == "neg":
        return -a[0] % P
    if op == "reduce128":
        return (a[0] + (b[0] << 64)) % P
    if op == "mul":
        return a[0] * b[0] % P
    if op in ("mul_pow2", "mul_pow2_rt", "shl96", "shl192", "shl_small_weak"):
        return (a[0] << s) % P
    if op == "add_weak":
        return (a[0] + b[0]) % P
    if op == "from_x_y32":
        return (_s64(a[0]) + (_s64(b[0]) << 32)) % P
    if op in ("acc_reduce", "cacc_reduce", "cacc_reduce_weak", "cacc_reduce_terms"):
        return sum(x * y for x, y in zip(a, b)) % P
    if op == "acc_add":
        return sum(x * y + x + y for x, y in zip(a, b)) % P
    if op == "to_mont":
        return a[0] * EPS % P
    if op == "from_mont":
        return a[0] * R_INV % P
    if op in ("fq3_mul", "s_mul3", "s_mul_w3"):
        return fq3_ref(a, b)
    if op in ("s_mad2_3", "sacc3", "fq3acc"):
        acc = (0, 0, 0)
        for i in range(m):
            t = fq3_ref(a[3 * i:3 * i + 3], b[3 * i:3 * i + 3])
            acc = tuple((x + y) % P for x, y in zip(acc, t))
        return acc
    raise KeyError(op)


def model(op, a, b, s, m):
    """(value, flags) of one case through the transliteration (host-and-device ops only)"""
    one = {"canon": lambda: canon(a[0]), "add": lambda: add(a[0], b[0]), "sub": lambda: sub(a[0], b[0]),
           "neg": lambda: neg(a[0]), "reduce128": lambda: reduce128(a[0], b[0]), "mul": lambda: mul(a[0], b[0]),
           "mul_pow2": lambda: mul_pow2(a[0], s), "mul_pow2_rt": lambda: mul_pow2(a[0], s),
           "shl96": lambda: shl96(a[0], s), "shl192": lambda: shl192(a[0], s),
           "shl_small_weak": lambda: shl_small_weak(a[0], s), "add_weak": lambda: add_weak(a[0], b[0]),
           "from_x_y32": lambda: from_x_y32(_s64(a[0]), _s64(b[0])), "to_mont": lambda: to_mont(a[0]),
           "from_mont": lambda: from_mont(a[0]), "fq3_mul": lambda: fq3_mul(a, b)}
    if op in one:
        return one[op]()
    f = {}
    if op in ("acc_reduce", "acc_add"):
        st = (0, 0, 0)
        for x, y in zip(a, b):
            st, g = acc_mad(st, x, y)
            _m(f, g)
            if op == "acc_add":
                for v in (x, y):
                    st, g = acc_add(st, v)
                    _m(f, g)
        want = sum(x * y + (x + y if op == "acc_add" else 0) for x, y in zip(a, b))
        assert acc_value(st) == want
        v, g = acc_reduce(st)
        if op == "acc_reduce":  # acc_add's census is acc_add's own decisions; the reduction is acc_reduce's
            _m(f, g)
        return v, f
    st = (0,) * 6
    for x, y in zip(a, b):
        st, g = cacc_mad(st, x, y)
        _m(f, g)
    assert cacc_value(st) == sum(x * y for x, y in zip(a, b))
    v, g = {"cacc_reduce": cacc_reduce, "cacc_reduce_weak": cacc_reduce_weak, "cacc_reduce_terms": cacc_reduce_terms}[op](st)
    _m(f, g)
    return v, f


# ------------------------------------------------------------------ vector sets
@dataclass
class VecSet:
    """n cases of one op: case i reads a[i m w : (i + 1) m w] (and b likewise), w words per
    element, with the shift s; the result is w words"""
    op: str
    a: list
    b: list | None
    s: int = 0
    m: int = 1
    w: int = 1
    n: int = field(init=False)

    def __post_init__(self):
        self.n = len(self.a) // (self.m * self.w)
        assert len(self.a) == self.n * self.m * self.w and (self.b is None or len(self.b) == len(self.a))

    def case(self, i):
        k = self.m * self.w
        return self.a[i * k:(i + 1) * k], (self.b[i * k:(i + 1) * k] if self.b is not None else None)


def signed_grid(nrand=4096):
    """the from_x_y32 grid of tests/test_gl_host.py: its edge pairs, then SplitMix64 pairs over
    every magnitude below 2^62; as (X, Y) signed"""
    L = (1 << 62) - 1
    edge = [0, 1, -1, L, -L, 1 << 32, -(1 << 32), (1 << 32) - 1, -((1 << 32) - 1), 1 << 48, -(1 << 48), 0x7FFFFFFF,
            -0x80000000, 0xFFFFFFFF00000001 >> 2]
    out = [(x, y) for x in edge for y in edge]
    st = [0x4C46]

    def nxt():
        st[0] = (st[0] + 0x9E3779B97F4A7C15) & M64
        z = st[0]
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)

    def pick():
        sh = nxt() % 63
        mag = nxt() >> (64 - sh) if sh else 0
        return -mag if nxt() & 1 else mag

    for _ in range(nrand):
        x = pick()
        y = pick()
        out.append((x, y))
    # directed: Y whose low word and high part sum across 2^32 both ways (c = 1, c = -1)
    for yl in (0, 1, M32 - 1, M32):
        for yh in (-(1 << 29), -2, -1, 0, 1, 2, (1 << 29) - 1):
            for x in (0, -L, L, -1):
                out.append((x, (yh << 32) + yl))
    return out


FROM_MONT_J = [2, 3, 4, 5, 7, 1 << 4, 1 << 8, (1 << 8) + 1, 1 << 16, (1 << 16) + 1, 1 << 24, 1 << 30]
RUN_LENGTHS = (1, 2, 3, 6, 9, 64, 4096)
RUNS_PER_LENGTH = {1: 2048, 2: 1024, 3: 1024, 6: 512, 9: 512, 64: 128, 4096: 8}


def acc_runs(m):
    """operand runs of m products: seeded draws from the any-u64
    set, then the all-(2^64 - 1) and all-(p - 1) runs, then directed runs"""
    _, any64 = edge_values()
    rng = random.Random(0x474D + 31 * m)
    k = m
    a, b = [], []
    for _ in range(RUNS_PER_LENGTH[m]):
        a += rng.choices(any64, k=k)
        b += rng.choices(any64, k=k)
    top = [x for x in any64 if x >> 62 == 3]
    for _ in range(max(8, RUNS_PER_LENGTH[m] // 8)):  # large operands: the counters and the top word fill up
        a += rng.choices(top, k=k)
        b += rng.choices(top, k=k)
    for v in (M64, P - 1):
        a += [v] * k
        b += [v] * k
    if 6 <= m <= 64:
        for pat in CACC_PATTERNS:
            for j in range(CENSUS_MIN):
                ra, rb = [0] * m, [0] * m
                for i, (x, y) in enumerate(pat):
                    ra[i], rb[i] = x, y
                ra[len(pat)], rb[len(pat)] = j, 1 + (j & 1) * (M32 - 1)  # a small product: only s0 (and s1) move
                a += ra
                b += rb
    return a, b


# directed product runs for cacc_reduce_weak's rare limb carries (operands from the edge set)
CACC_PATTERNS = (
    # 4 x 2^126 wraps s2 to 0 with c2 = 1 and every other limb 0: uh = 0 < x4, the borrow b (and b2)
    ((1 << 63, 1 << 63),) * 4,
    # the same with s0l = 2^32 - 1, so the low word absorbs the borrow without b2
    ((1 << 63, 1 << 63),) * 4 + ((M32, 1),),
    # c0 = 1 from two (2^32-1)^2 in s0, and s2 = 2^64 - 1: y = 2^32 - 1 carries with c0 (kb), and z = 2^32 - 1
    # carries with kb (kd)
    ((M32, M32), (M32, M32), (P - 1, P - 1), (1 << 33, P - 1)),
    # s2 = 2^64 - 1 and c1 = 1 from two (2^32-1)^2 in s1: z = s2h + c1 carries (kc)
    ((P - 1, P - 1), (1 << 33, P - 1), (M32, P - 1), (M32, P - 1)),
)


def acc_add_directed(m):
    """runs for acc_add's carry into top: (2^64-1)^2 + 2 (2^64-1) fills lo and hi, then a
    further + 1 ripples through both words"""
    a, b = [], []
    if m >= 2:
        for j in range(1, m):
            for tail in (0, 1):
                ra, rb = [0] * m, [0] * m
                ra[0] = rb[0] = M64
                rb[j] = 1
                if j + 1 < m:
                    ra[j + 1] = tail
                a += ra
                b += rb
                if len(a) >= 16 * m:
                    return a, b
    return a, b


@functools.lru_cache(maxsize=None)
def vector_sets():
    """every VecSet the host and device checks run, in a fixed order"""
    can, any64 = edge_values()
    sets = []
    pc_a = [x for x in can for _ in can]
    pc_b = [y for _ in can for y in can]
    pa_a = [x for x in any64 for _ in any64]
    pa_b = [y for _ in any64 for y in any64]
    sets.append(VecSet("canon", list(any64), None))
    sets.append(VecSet("neg", list(can) + [0] * CENSUS_MIN, None))  # neg's one special case is a = 0
    sets.append(VecSet("add", pc_a, pc_b))
    sets.append(VecSet("sub", pc_a, pc_b))
    sets.append(VecSet("reduce128", pa_a, pa_b))
    sets.append(VecSet("mul", pa_a, pa_b))
    sets.append(VecSet("add_weak", [x for x in any64 for _ in can], [y for _ in any64 for y in can]))
    for s in range(192):
        sets.append(VecSet("mul_pow2", list(any64), None, s=s))
        sets.append(VecSet("mul_pow2_rt", list(any64), None, s=s))
        sets.append(VecSet("shl192", list(can), None, s=s))
    for s in range(96):
        sets.append(VecSet("shl96", list(can), None, s=s))
    for s in range(1, 32):
        sets.append(VecSet("shl_small_weak", list(any64), None, s=s))
    g = signed_grid()
    sets.append(VecSet("from_x_y32", [x & M64 for x, _ in g], [y & M64 for _, y in g]))
    sets.append(VecSet("to_mont", list(any64), None))
    # from_mont's reduce128 lands in [p, 2^64) on the Montgomery forms of small j: j (2^32 - 1)
    sets.append(VecSet("from_mont", list(any64) + [j * EPS for j in FROM_MONT_J], None))
    for m in RUN_LENGTHS:
        a, b = acc_runs(m)
        for op in ("acc_reduce", "cacc_reduce", "cacc_reduce_weak", "cacc_reduce_terms"):
            sets.append(VecSet(op, a, b, m=m))
        da, db = acc_add_directed(m)
        sets.append(VecSet("acc_add", a + da, b + db, m=m))
    rng = random.Random(0x4671)
    n3 = 4099  # ends inside a block of the probe
    sets.append(VecSet("fq3_mul", rng.choices(can, k=3 * n3), rng.choices(can, k=3 * n3), w=3))
    sets.append(VecSet("s_mul3", rng.choices(can, k=3 * n3), rng.choices(can, k=3 * n3), w=3))
    # s_mul_w: the left operand any u64 (weakly reduced), the right one canonical
    sets.append(VecSet("s_mul_w3", rng.choices(any64, k=3 * n3), rng.choices(can, k=3 * n3), w=3))
    sets.append(VecSet("s_mad2_3", rng.choices(can, k=6 * n3), rng.choices(can, k=6 * n3), m=2, w=3))
    for m in (1, 3, 64):
        for op in ("sacc3", "fq3acc"):
            k = 3 * m * (n3 // m if m > 1 else n3 // 4)
            a, b = rng.choices(can, k=k), rng.choices(can, k=k)
            a += [P - 1] * (3 * m)
            b += [P - 1] * (3 * m)
            sets.append(VecSet(op, a, b, m=m, w=3))
    return tuple(sets)


@functools.lru_cache(maxsize=None)
def expected():
    """ref() of every case of every vector set, in vector_sets() order (computed once)"""
    return tuple([ref(vs.op, *vs.case(i), vs.s, vs.m) for i in range(vs.n)] for vs in vector_sets())


def shift_range(op):
    return {"mul_pow2": range(192), "mul_pow2_rt": range(192), "shl192": range(192), "shl96": range(96),
            "shl_small_weak": range(1, 32)}.get(op)


# ------------------------------------------------------------------ the census
@functools.lru_cache(maxsize=None)
def census():
    """over vector_sets(): per primitive the case count, the transliteration's mismatches with
    ref() (congruence for the weak ops), and per flag [times set, times clear]"""
    count, bad, flags = {}, {}, {}
    for vs in vector_sets():
        if vs.op in DEVICE_ONLY_OPS:
            count[vs.op] = count.get(vs.op, 0) + vs.n
            continue
        fl = flags.setdefault(vs.op, {})
        for i in range(vs.n):
            a, b = vs.case(i)
            v, f = model(vs.op, a, b, vs.s, vs.m)
            want = ref(vs.op, a, b, vs.s, vs.m)
            if vs.op in WEAK_OPS:
                ok = 0 <= v <= M64 and v % P == want
            else:
                ok = v == want
            if not ok:
                bad.setdefault(vs.op, []).append((vs.s, vs.m, i, v, want))
            for k, t in f.items():
                e = fl.setdefault(k, [0, 0])
                e[0 if t else 1] += 1
        count[vs.op] = count.get(vs.op, 0) + vs.n
    return count, bad, flags


def census_report():
    count, bad, flags = census()
    lines = []
    for op in count:
        lines.append(f"{op}: {count[op]} vectors, {len(bad.get(op, []))} model mismatches")
        for k, (st, cl) in sorted(flags.get(op, {}).items()):
            tag = "  (proven unreachable)" if unreachable(op, k) else ""
            lines.append(f"    {k}: set {st}, clear {cl}{tag}")
    return "\n".join(lines)


if __name__ == "__main__":
    print(census_report())
