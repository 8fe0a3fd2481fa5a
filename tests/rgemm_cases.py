"""Inputs and float64 references of the row-GEMM shape tests
(test_gpu_rgemm_shapes.py on the device, test_rgemm_cases.py on the CPU alone):
mmpde_rgemm (csrc/rgemm.hip: the weight-stationary form and the 128 x 128 tile
form), mmpde_rgemm_tn, mmpde_rows_small (csrc/rows_small.hip) and the
dispatcher ops.LinearRows, at their tile, grid and segment edges.

A case is a dict: `bufs` (name -> flat fp32 CPU tensor, never modified) plus the
call's description, every pointer a ref = (buffer name, offset in floats).  The
references are the formulas of include/mmpde_hip.h on strided views of the
flat buffers, in float64 (or, for the CPU floor check, float32).

Every input buffer starts as NaN and only what the call may use is filled
(seeded randn, weights scaled by 1 / sqrt(K)): pad columns, rows at and beyond
m, the columns of xs at and beyond ns, the floats in front of an offset
pointer and the masked-off elements of a masked operand stay NaN.  Masks are
randn with a planted share of 0.0, -0.0 and 2^-126.  Every output buffer starts
as SENT (accumulating regions as randn); what the call does not own must come
back bitwise unchanged.

Bars (tests/test_gpu_rgemm.py): mmpde_rgemm and mmpde_rows_small 1e-5 of
max|ref| for a total K <= 260, 2e-5 above; mmpde_rgemm_tn 2e-5 of max|ref| (of
the summands' scale where a column cancels by construction); max|ref| = 0
requires an exact 0.  test_rgemm_cases.py holds the float32 evaluation of every
reference to a quarter of its bar.
"""
import functools
import math

import torch

from mmpde_amd import _lib as L
from mmpde_amd import rows

NT, NN = L.RGEMM_NT, L.RGEMM_NN
LAYOUT = {NT: "NT", NN: "NN"}
SENT = 777.125
TINY = 2.0 ** -126
FLOOR_SHARE = 0.25                   # the fp32 CPU evaluation must stay within this share of the bar


# --------------------------------------------------------------------------- buffers
def view(flat, off, nrows, ncols, ld):
    return flat.as_strided((nrows, ncols), (ld, 1), off)


def off(ref, k):
    return (ref[0], ref[1] + k)


def mask_values(g, nrows, ncols):
    v = torch.randn(nrows, ncols, generator=g)
    r = torch.rand(nrows, ncols, generator=g)
    v[r < 0.1] = 0.0
    v[(r >= 0.1) & (r < 0.2)] = -0.0
    v[(r >= 0.2) & (r < 0.3)] = TINY
    return v


class Bufs:
    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)
        self.t = {}

    def alloc(self, name, nrows, ld, front=4, fill=float("nan")):
        """front floats, nrows + 2 rows of ld, 8 more floats; returns the ref of row 0."""
        self.t[name] = torch.full((front + (nrows + 2) * ld + 8,), fill, dtype=torch.float32)
        return (name, front)

    def fill(self, ref, nrows, ncols, ld, scale=1.0, values=None):
        v = torch.randn(nrows, ncols, generator=self.g) * scale if values is None else values
        view(self.t[ref[0]], ref[1], nrows, ncols, ld).copy_(v)
        return ref

    def inp(self, name, nrows, ncols, ld=None, front=4, scale=1.0):
        ld = ld or ncols
        return self.fill(self.alloc(name, nrows, ld, front), nrows, ncols, ld, scale)

    def mask(self, name, nrows, ncols, ld=None, front=4, all_off=False):
        ld = ld or ncols
        v = mask_values(self.g, nrows, ncols)
        if all_off:
            v = torch.where(v > 0, -v, v)
        return self.fill(self.alloc(name, nrows, ld, front), nrows, ncols, ld, values=v)

    def out(self, name, nrows, ld, front=4):
        return self.alloc(name, nrows, ld, front, SENT)

    def nan_where_off(self, ref, mref, nrows, ncols, ld):
        a = view(self.t[ref[0]], ref[1], nrows, ncols, ld)
        a[~(view(self.t[mref[0]], mref[1], nrows, ncols, ld) > 0)] = float("nan")


def _v(c, ref, nrows, ncols, ld, dtype):
    return view(c["bufs"][ref[0]], ref[1], nrows, ncols, ld).to(dtype)


def _region(ref, nrows, ncols, ld, values, grp, scale=None):
    return dict(ref=ref, rows=nrows, cols=ncols, ld=ld, values=values, grp=grp, scale=scale)


# --------------------------------------------------------------------------- mmpde_rgemm
PART_DEFAULTS = dict(wc=0, wk=0, bias=None, omask=None, ldom=0, acc=False, ns=0, xw=None, xscale=1.0)


def rgemm_case(b, name, group, m, kh, layout, w, ldw, a, lda, parts, amask=(None, None), relu=False, xs=None,
               ldxs=0, ldxw=0):
    parts = [dict(PART_DEFAULTS, **p) for p in parts]
    k = 2 * kh + max(p["ns"] for p in parts)
    return dict(kind="rgemm", name=name, group=group, bufs=b.t, m=m, kh=kh, layout=layout, w=w, ldw=ldw, a=a,
                lda=lda, parts=parts, amask=amask, relu=relu, xs=xs, ldxs=ldxs, ldxw=ldxw,
                bar=1e-5 if k <= 260 else 2e-5)


def rgemm_reference(c, dtype=torch.float64):
    """y = sum_h A_h B_h(p) + bias + xscale xs[:, :ns] XW; relu; omask select; out_old + y."""
    m, kh, ldw = c["m"], c["kh"], c["ldw"]
    regions = []
    for i, p in enumerate(c["parts"]):
        nc = p["ncols"]
        y = torch.zeros(m, nc, dtype=dtype)
        for h in range(2 if kh > 0 else 0):
            a = _v(c, c["a"][h], m, kh, c["lda"][h], dtype)
            if c["amask"][h] is not None:
                a = torch.where(_v(c, c["amask"][h], m, kh, c["lda"][h], dtype) > 0, a, torch.zeros_like(a))
            if c["layout"] == NT:
                bm = _v(c, off(c["w"][h], p["wc"] * ldw + p["wk"]), nc, kh, ldw, dtype).t()
            else:
                bm = _v(c, off(c["w"][h], p["wk"] * ldw + p["wc"]), kh, nc, ldw, dtype)
            y = y + a @ bm
        if p["bias"] is not None:
            y = y + _v(c, p["bias"], 1, nc, nc, dtype)
        if p["ns"] > 0:
            x = _v(c, c["xs"], m, p["ns"], c["ldxs"], dtype)
            xw = _v(c, p["xw"], nc, p["ns"], c["ldxw"], dtype).t() if c["layout"] == NT else \
                _v(c, p["xw"], p["ns"], nc, c["ldxw"], dtype)
            y = y + p["xscale"] * (x @ xw)
        if c["relu"]:
            y = torch.relu(y)
        if p["omask"] is not None:
            y = torch.where(_v(c, p["omask"], m, nc, p["ldom"], dtype) > 0, y, torch.zeros_like(y))
        if p["acc"]:
            y = _v(c, p["out"], m, nc, p["ldo"], dtype) + y
        regions.append(_region(p["out"], m, nc, p["ldo"], y, f"part{i}"))
    return regions


def rgemm_form(c, base=lambda name: 0):
    """The kernel instantiation mmpde_rgemm picks (its dispatch, restated);
    base(name): the buffer's address (the CPU side assumes 16-byte bases)."""
    def al16(ref):
        return (base(ref[0]) + 4 * ref[1]) % 16 == 0

    kh, nt = c["kh"], c["layout"] == NT
    xs = any(p["ns"] > 0 for p in c["parts"])
    vec = kh % 4 == 0
    if kh > 0:
        for h in range(2):
            vec = vec and al16(c["a"][h]) and c["lda"][h] % 4 == 0 and \
                (c["amask"][h] is None or al16(c["amask"][h]))
            if nt:
                vec = vec and al16(c["w"][h]) and c["ldw"] % 4 == 0
        if nt:
            vec = vec and all(p["wk"] % 4 == 0 for p in c["parts"])
    am = kh > 0 and c["amask"][0] is not None
    if vec and kh in (32, 64, 128):
        return ("ws", LAYOUT[c["layout"]], kh, am, xs)
    return ("tile", LAYOUT[c["layout"]], vec, am, xs)


def ws_slots(kh, nparts, cus):
    return max(1, (1 if kh == 128 else 2) * cus // nparts)


def multi_tile_rows(kh, nparts, cus):
    """Some workgroups take three 32-row tiles, the rest two; the last tile is partial."""
    return 32 * (2 * ws_slots(kh, nparts, cus) + 1) + 5


# The seven mmpde_rgemm launches of GnnLayerTrain (gnn_2d.py), and the ncols = 4
# sibling of the sixth, with the production offsets, strides and part tables.
PROD = {1: (64, 2), 2: (128, 1), 3: (64, 1), 4: (64, 1), 5: (64, 2), 6: (128, 1), "6s": (128, 1), 7: (64, 1)}


def production(idx, n, seed=0):
    b = Bufs(1000 + 37 * (list(PROD).index(idx)) + n + seed)
    name = f"prod{idx}-n{n}"
    s260, s257, s128 = 260 ** -0.5, 257 ** -0.5, 128 ** -0.5

    def out(nm, ld=128):
        return b.out(nm, n, ld)

    if idx == 1:
        w1 = b.inp("W1", 128, 260, scale=s260)
        h, ext = b.inp("h", n, 128), b.inp("ext", n, 4)
        parts = [dict(out=out("a"), ldo=128, ncols=128, bias=b.inp("B1", 1, 128), ns=4, xw=off(w1, 256)),
                 dict(out=out("b"), ldo=128, wk=128, ncols=128, ns=3, xw=off(w1, 256), xscale=-1.0)]
        return rgemm_case(b, name, "A", n, 64, NT, (w1, off(w1, 64)), 260, (h, off(h, 64)), (128, 128), parts,
                          xs=ext, ldxs=4, ldxw=260)
    if idx == 2:
        u1 = b.fill(b.alloc("U1", 128, 260), 128, 257, 260, s257)
        h, mean = b.inp("h", n, 128), b.inp("mean", n, 128)
        t = b.fill(off(b.alloc("ext", n, 4), 3), n, 1, 4)
        parts = [dict(out=out("v"), ldo=128, ncols=128, bias=b.inp("C1", 1, 128), ns=1, xw=off(u1, 256))]
        return rgemm_case(b, name, "A", n, 128, NT, (u1, off(u1, 128)), 260, (h, mean), (128, 128), parts,
                          relu=True, xs=t, ldxs=4, ldxw=260)
    if idx == 3:
        u2, v = b.inp("U2", 128, 128, scale=s128), b.inp("v", n, 128)
        parts = [dict(out=out("upd"), ldo=128, ncols=128, bias=b.inp("C2", 1, 128))]
        return rgemm_case(b, name, "A", n, 64, NT, (u2, off(u2, 64)), 128, (v, off(v, 64)), (128, 128), parts,
                          relu=True)
    if idx == 4:
        u2, dx = b.inp("U2", 128, 128, scale=s128), b.inp("dx", n, 128)
        upd, v = b.mask("upd", n, 128), b.mask("v", n, 128)
        b.nan_where_off(dx, upd, n, 128, 128)
        parts = [dict(out=out("dv"), ldo=128, ncols=128, omask=v, ldom=128)]
        return rgemm_case(b, name, "A", n, 64, NN, (u2, off(u2, 64 * 128)), 128, (dx, off(dx, 64)), (128, 128),
                          parts, amask=(upd, off(upd, 64)))
    if idx == 5:
        u1 = b.fill(b.alloc("U1", 128, 260), 128, 256, 260, s128)
        dv = b.inp("dv", n, 128)
        parts = [dict(out=b.fill(out("dx"), n, 128, 128), ldo=128, wc=0, ncols=128, acc=True),
                 dict(out=out("dmean"), ldo=128, wc=128, ncols=128)]
        return rgemm_case(b, name, "A", n, 64, NN, (u1, off(u1, 64 * 260)), 260, (dv, off(dv, 64)), (128, 128),
                          parts)
    if idx in (6, "6s"):
        da, db = b.inp("da", n, 128), b.inp("db", n, 128)
    if idx == 6:
        w1 = b.fill(b.alloc("W1", 128, 260), 128, 256, 260, 256 ** -0.5)
        parts = [dict(out=b.fill(out("dx"), n, 128, 128), ldo=128, wc=0, ncols=128, acc=True)]
        return rgemm_case(b, name, "A", n, 128, NN, (w1, off(w1, 128)), 260, (da, db), (128, 128), parts)
    if idx == "6s":
        w1 = b.fill(off(b.alloc("W1", 128, 260), 256), 128, 4, 260, 256 ** -0.5)
        nwp = b.fill(off(b.alloc("nwp", 128, 260), 256), 128, 3, 260, 256 ** -0.5)
        b.fill(off(nwp, 3), 128, 1, 260, values=torch.zeros(128, 1))
        parts = [dict(out=out("dext", 4), ldo=4, ncols=4)]
        return rgemm_case(b, name, "A", n, 128, NN, (w1, nwp), 260, (da, db), (128, 128), parts)
    assert idx == 7
    u1 = b.fill(off(b.alloc("U1", 128, 260), 256), 128, 1, 260, s128)
    dv = b.inp("dv", n, 128)
    parts = [dict(out=b.fill(off(out("dext", 4), 3), n, 1, 4), ldo=4, ncols=1, acc=True)]
    return rgemm_case(b, name, "A", n, 64, NN, (u1, off(u1, 64 * 260)), 260, (dv, off(dv, 64)), (128, 128), parts)


GP_DEFAULTS = dict(ns=0, bias=False, omask=False, acc=False, wc=0, wk=0, xscale=1.0)


def generic(name, group, seed, layout, kh, n, parts, am=False, relu=False, variant="vec"):
    """mmpde_rgemm on buffers of the test's own: two input tensors of different
    padded strides, padded weights, xs an offset pointer of stride 6.
    variant: oddlda (odd row strides), offbase (a[0] one float off 16 bytes)."""
    b = Bufs(seed)
    gp = [dict(GP_DEFAULTS, **p) for p in parts]
    nsmax = max(p["ns"] for p in gp)
    ws = (2 * kh + nsmax) ** -0.5
    nt = layout == NT
    w, a, amask, lda = (None, None), (None, None), (None, None), (0, 0)
    ldw = 0
    if kh > 0:
        lda = (kh + 5, kh + 7) if variant == "oddlda" else (kh + 4, kh + 8)
        a = tuple(b.inp(f"a{h}", n, kh, lda[h], front=5 if (variant == "offbase" and h == 0) else 4)
                  for h in range(2))
        if am:
            amask = tuple(b.mask(f"am{h}", n, kh, lda[h], front=a[h][1]) for h in range(2))
            for h in range(2):
                b.nan_where_off(a[h], amask[h], n, kh, lda[h])
        wrows = max(p["wc"] + p["ncols"] for p in gp) if nt else max(p["wk"] for p in gp) + kh
        wcols = max(p["wk"] for p in gp) + kh if nt else max(p["wc"] + p["ncols"] for p in gp)
        ldw = (wcols + 3) // 4 * 4 + 4 if nt else wcols + 3
        w = tuple(b.alloc(f"w{h}", wrows, ldw) for h in range(2))
        for h in range(2):
            for p in gp:
                if nt:
                    b.fill(off(w[h], p["wc"] * ldw + p["wk"]), p["ncols"], kh, ldw, ws)
                else:
                    b.fill(off(w[h], p["wk"] * ldw + p["wc"]), kh, p["ncols"], ldw, ws)
    xs, ldxs, ldxw = None, 0, 0
    if nsmax:
        xs, ldxs, ldxw = b.fill(b.alloc("xs", n, 6, front=5), n, nsmax, 6), 6, 7 if nt else 133
    out = []
    for i, p in enumerate(gp):
        nc = p["ncols"]
        q = dict(ncols=nc, ldo=nc + 5, wc=p["wc"], wk=p["wk"], acc=p["acc"], ns=p["ns"], xscale=p["xscale"])
        q["out"] = b.out(f"out{i}", n, nc + 5, front=3)
        if p["acc"]:
            b.fill(q["out"], n, nc, nc + 5)
        if p["bias"]:
            q["bias"] = b.inp(f"bias{i}", 1, nc)
        if p["omask"]:
            q["omask"], q["ldom"] = b.mask(f"om{i}", n, nc, nc + 3, front=1, all_off=p["omask"] == "off"), nc + 3
        if p["ns"]:
            q["xw"] = b.inp(f"xw{i}", nc, p["ns"], ldxw, scale=ws) if nt else b.inp(f"xw{i}", p["ns"], nc, ldxw,
                                                                                   scale=ws)
        out.append(q)
    return rgemm_case(b, name, group, n, kh, layout, w, ldw, a, lda, out, amask=amask, relu=relu, xs=xs,
                      ldxs=ldxs, ldxw=ldxw)


ROWS_A = (1, 31, 32, 33, 65)


def cases_a(cus):
    """name -> builder of the weight-stationary cases."""
    t = {}
    for idx, (kh, nparts) in PROD.items():
        for n in ROWS_A:
            t[f"prod{idx}-n{n}"] = functools.partial(production, idx, n)
        t[f"prod{idx}-multi"] = functools.partial(production, idx, multi_tile_rows(kh, nparts, cus))
    # kh = 32: a partial wave and a wave without columns; a single column; one full wave
    for lay in (NT, NN):
        ln = LAYOUT[lay]
        t[f"ws32-{ln}-c33-100"] = functools.partial(
            generic, f"ws32-{ln}-c33-100", "A", 50 + lay, lay, 32, 65,
            [dict(ncols=33, ns=2, bias=True), dict(ncols=100, wc=40, wk=4, acc=True, ns=4, xscale=-1.0)])
        t[f"ws32-{ln}-c1-32"] = functools.partial(
            generic, f"ws32-{ln}-c1-32", "A", 52 + lay, lay, 32, 33,
            [dict(ncols=1, omask=True), dict(ncols=32, wc=1, bias=True)], am=True, relu=True)
        # one part with a small segment, one without (xs an offset pointer, NaN in front of it)
        for ns in ((4, 0), (0, 3)):
            nm = f"ws64-{ln}-ns{ns[0]}{ns[1]}"
            t[nm] = functools.partial(generic, nm, "A", 54 + lay + 2 * ns[0], lay, 64, 33,
                                      [dict(ncols=128, ns=ns[0], bias=True), dict(ncols=100, ns=ns[1], wc=128)])
        # every instantiation once more on padded buffers, two tiles and a partial one
        for kh in (32, 64, 128):
            for am in (False, True):
                for xs in (False, True):
                    nm = f"wsx-{ln}-k{kh}-am{int(am)}-xs{int(xs)}"
                    parts = [dict(ncols=128 if kh == 64 else 77, ns=3 if xs else 0, bias=am, omask=xs, acc=not am)]
                    t[nm] = functools.partial(generic, nm, "A", 60 + kh + 2 * am + xs + lay, lay, kh, 65, parts,
                                              am=am, relu=xs and am)
    return t


ROWS_B = (1, 63, 64, 65, 127, 128, 129, 300)
COLS_B = (1, 31, 33, 64, 65, 100, 128)
TILE_KH = [(4, "vec"), (8, "vec"), (36, "vec"), (132, "vec"), (148, "vec"),
           (1, "plain"), (2, "plain"), (3, "plain"), (5, "plain"), (37, "plain"),
           (36, "oddlda"), (36, "offbase"), (64, "wk2"), (0, "ns1"), (0, "ns4")]


def cases_b():
    """name -> builder of the 128 x 128 tile-kernel cases (kh outside {32, 64,
    128}, or operands the float4 loads cannot take)."""
    t = {}
    i = 0
    for lay in (NT, NN):
        for j, (kh, variant) in enumerate(TILE_KH):
            if variant == "wk2" and lay == NN:
                continue                              # wk is a row offset there: no effect on the form
            n, nc = ROWS_B[i % 8], COLS_B[i % 7]
            am = kh > 0 and bool(j & 1)
            xs = kh == 0 or bool(j & 2) ^ (variant in ("oddlda", "offbase"))
            ns = {"ns1": 1, "ns4": 4}.get(variant, 1 + i % 4) if xs else 0
            wk = 2 if variant == "wk2" else 0
            parts = [dict(ncols=nc, ns=ns, bias=i % 2 == 0, omask=i % 3 == 0, acc=i % 4 == 1, wk=wk,
                          xscale=(-1.0, 0.5, 1.0)[i % 3])]
            if i % 3 == 1:                             # two parts
                parts.append(dict(ncols=COLS_B[(i + 3) % 7], ns=0 if kh else ns, wc=5, wk=wk + (4 if kh else 0),
                                  acc=i % 2 == 0, bias=True))
            nm = f"tile-{LAYOUT[lay]}-k{kh}-{variant}-n{n}-c{nc}"
            t[nm] = functools.partial(generic, nm, "B", 200 + i, lay, kh, n, parts, am=am, relu=i % 4 == 2,
                                      variant=variant)
            i += 1
    # a fully masked output: exact zeros
    t["tile-NN-k36-masked-off"] = functools.partial(generic, "tile-NN-k36-masked-off", "B", 299, NN, 36, 65,
                                                    [dict(ncols=33, omask="off", bias=True)])
    return t


# which case covers which rgemm_kernel<LAYOUT, VEC, AMASK, XS> (test_rgemm_cases.py
# checks every entry against rgemm_form and that the 16 are all there)
TILE_COVERAGE = {
    ("NT", True, False, False): "tile-NT-k4-vec-n1-c1",
    ("NT", True, True, False): "tile-NT-k8-vec-n63-c31",
    ("NT", True, False, True): "tile-NT-k36-vec-n64-c33",
    ("NT", True, True, True): "tile-NT-k132-vec-n65-c64",
    ("NT", False, False, False): "tile-NT-k5-plain-n1-c31",
    ("NT", False, True, False): "tile-NT-k1-plain-n128-c100",
    ("NT", False, False, True): "tile-NT-k2-plain-n129-c128",
    ("NT", False, True, True): "tile-NT-k3-plain-n300-c1",
    ("NN", True, False, False): "tile-NN-k4-vec-n300-c31",
    ("NN", True, True, False): "tile-NN-k8-vec-n1-c33",
    ("NN", True, False, True): "tile-NN-k36-vec-n63-c64",
    ("NN", True, True, True): "tile-NN-k132-vec-n64-c65",
    ("NN", False, False, False): "tile-NN-k5-plain-n300-c33",
    ("NN", False, True, False): "tile-NN-k1-plain-n127-c128",
    ("NN", False, False, True): "tile-NN-k2-plain-n128-c1",
    ("NN", False, True, True): "tile-NN-k3-plain-n129-c31",
}


# --------------------------------------------------------------------------- mmpde_rgemm_tn
LDDW = 257


def tn_case(name, seed, m, chunk, gcols, kxs, ns=0, sign=1.0, acc=False, db=True, gmask=False, variant="vec",
            cancel=False, all_off=False):
    """variant: vec (even strides, 8-byte pointers), oddldg, oddldx, offptr (g one float off)."""
    b = Bufs(seed)
    ldg = gcols + 3 if (gcols + 3) % 2 else gcols + 4
    if variant != "oddldg":
        ldg = (gcols + 3) // 2 * 2
    g = b.inp("g", m, gcols, ldg, front=5 if variant == "offptr" else 4)
    gm = None
    if gmask:
        gm = b.mask("gm", m, gcols, ldg, all_off=all_off)
        b.nan_where_off(g, gm, m, gcols, ldg)
    segs, col = [], 2
    for s, kx in enumerate(kxs):
        ldx = (kx + 3) // 2 * 2
        if variant == "oddldx" and s == 0:
            ldx = kx + 3 if (kx + 3) % 2 else kx + 4
        segs.append((b.inp(f"x{s}", m, kx, ldx), ldx, kx, col))
        col += kx + 3
    dwcol_s = col + 1
    assert dwcol_s + ns <= LDDW
    xs = b.fill(b.alloc("xs", m, 6, front=5), m, ns, 6) if ns else None
    dw = b.out("dw", gcols, LDDW)
    c = dict(kind="tn", name=name, group="C", bufs=b.t, m=m, chunk=chunk, gcols=gcols, g=g, gmask=gm, ldg=ldg,
             segs=segs, xs=xs, ldxs=6 if ns else 0, ns=ns, dwcol_s=dwcol_s, sign=sign, acc=acc, dw=dw,
             db=b.out("db", 1, gcols + 3) if db else None, cancel=cancel, bar=2e-5)
    if acc and ns:
        old = None
        if cancel:                                    # the stored copy the signed sum cancels against
            old = tn_products(c, torch.float64)[0].float()
        b.fill(off(dw, dwcol_s), gcols, ns, LDDW, values=old)
    return c


def tn_products(c, dtype):
    m, gc = c["m"], c["gcols"]
    g = _v(c, c["g"], m, gc, c["ldg"], dtype)
    if c["gmask"] is not None:
        g = torch.where(_v(c, c["gmask"], m, gc, c["ldg"], dtype) > 0, g, torch.zeros_like(g))
    x = _v(c, c["xs"], m, c["ns"], c["ldxs"], dtype) if c["ns"] else torch.zeros(m, 0, dtype=dtype)
    return g.t() @ x, g.abs().t() @ x.abs(), g


def tn_reference(c, dtype=torch.float64):
    """G = where(gmask > 0, g, 0); dW segments G^T X_s; the small segment with
    sign_s / accumulate_s; db = G.sum(0)."""
    gc = c["gcols"]
    small, summands, g = tn_products(c, dtype)
    regions = []
    for x, ldx, kx, dwcol in c["segs"]:
        regions.append(_region(off(c["dw"], dwcol), gc, kx, LDDW, g.t() @ _v(c, x, c["m"], kx, ldx, dtype), "dw"))
    if c["ns"]:
        ref = off(c["dw"], c["dwcol_s"])
        y = c["sign"] * small
        if c["acc"]:
            y = _v(c, ref, gc, c["ns"], LDDW, dtype) + y
        regions.append(_region(ref, gc, c["ns"], LDDW, y, "dw-small" if c["cancel"] else "dw",
                               summands.max().item() if c["cancel"] else None))
    if c["db"] is not None:
        regions.append(_region(c["db"], 1, gc, gc + 3, g.sum(0, keepdim=True), "db"))
    return regions


def tn_form(c, base=lambda name: 0):
    """rgemm_tn_partial_kernel<GMASK, VEC, XS> as mmpde_rgemm_tn picks it."""
    def al8(ref):
        return (base(ref[0]) + 4 * ref[1]) % 8 == 0

    vec = c["gcols"] >= 2 and c["ldg"] % 2 == 0 and al8(c["g"]) and (c["gmask"] is None or al8(c["gmask"]))
    for x, ldx, kx, _ in c["segs"]:
        vec = vec and kx >= 2 and ldx % 2 == 0 and al8(x)
    return (c["gmask"] is not None, vec, c["ns"] > 0)


ROWS_C = (1, 2, 3, 63, 64, 65, 129, 255, 256, 257, 511, 513, 256 * 9 + 1)
GCOLS_C = (1, 2, 5, 63, 64, 65, 127, 128)
SEGS_C = ([1], [2], [3], [63], [64], [65], [128], [131], [64, 3], [65, 128], [131, 63], [1, 2, 3], [63, 64, 65],
          [128, 1, 2])


def cases_c():
    t = {}

    def add(nm, *a, **k):
        t[nm] = functools.partial(tn_case, nm, 300 + len(t), *a, **k)

    for i, m in enumerate(ROWS_C):
        add(f"tn-m{m}-g{GCOLS_C[i % 8]}-k{'_'.join(map(str, SEGS_C[i]))}-ns{i % 5}", m, 256, GCOLS_C[i % 8],
            SEGS_C[i], ns=i % 5, sign=-1.0 if i & 1 else 1.0, acc=bool(i & 2), db=i % 3 != 2, gmask=bool(i & 4))
    add("tn-m300-g63-k128_1_2-ns2", 300, 256, 63, SEGS_C[13], ns=2, sign=-1.0, acc=True, gmask=True)
    # every instantiation by name: VEC with an odd gcols and an odd kx (the
    # clamped pairs start at odd columns), non-VEC from a stride or a pointer
    for i, (gm, xs) in enumerate(((False, False), (False, True), (True, False), (True, True))):
        add(f"tn-vec-gm{int(gm)}-xs{int(xs)}", 131, 256, 5, [3, 65], ns=3 * xs, gmask=gm, db=not gm,
            sign=-1.0, acc=gm)
        var = ("oddldg", "oddldx", "offptr", "oddldg")[i]
        add(f"tn-{var}-gm{int(gm)}-xs{int(xs)}", 67, 256, 64 - i, [64, 2 + i], ns=4 * xs, gmask=gm, db=gm,
            variant=var)
    add("tn-offptr-g127-k63", 258, 256, 127, [63], ns=1, variant="offptr")
    # chunk variants: 65 chunks (the reduce's second trip), a wave without rows,
    # the rolled loop at 33 and 128 steps per wave
    add("tn-chunk2-m1", 1, 2, 2, [2], ns=1, gmask=True)
    add("tn-chunk2-m5", 5, 2, 65, [3], ns=4, sign=-1.0)
    add("tn-chunk2-m130", 130, 2, 5, [65], ns=2, gmask=True, acc=True)
    add("tn-chunk6-m17", 17, 6, 64, [63, 64, 65], ns=3, gmask=True)
    add("tn-chunk258-m261", 261, 258, 127, [131], ns=4, gmask=True, acc=True, sign=-1.0)
    add("tn-chunk1024-m1027", 1027, 1024, 128, [128, 1, 2], ns=1, db=False)
    add("tn-chunk258-m261-nogm", 261, 258, 65, [64, 3], ns=0)
    # columns that cancel by construction, judged against the summands' scale
    add("tn-cancel", 513, 256, 64, [64], ns=4, sign=-1.0, acc=True, cancel=True, gmask=True)
    # fully masked: exact zeros
    add("tn-masked-off", 65, 256, 33, [5], ns=2, gmask=True, all_off=True)
    return t


# --------------------------------------------------------------------------- mmpde_rows_small
def small_case(name, seed, layout, kin, kout, n, bias=False, ldx_pad=0, xfront=4, ldy_pad=0, yfront=4):
    """kin inputs and kout outputs per row: NT W [kout, kin] (+ bias), NN W [kin, kout]."""
    b = Bufs(seed)
    ki, no = (kin, kout) if layout == NT else (kout, kin)
    ldx, ldy, ldw = kin + ldx_pad, kout + ldy_pad, ki + 1
    return dict(kind="small", name=name, group="D", bufs=b.t, n=n, ki=ki, no=no, kin=kin, kout=kout, layout=layout,
                x=b.inp("x", n, kin, ldx, front=xfront), ldx=ldx, w=b.inp("w", no, ki, ldw, scale=kin ** -0.5),
                ldw=ldw, bias=b.inp("bias", 1, kout) if bias else None, y=b.out("y", n, ldy, front=yfront),
                ldy=ldy, bar=1e-5)


def small_reference(c, dtype=torch.float64):
    """NT x W^T + b; NN x W."""
    x = _v(c, c["x"], c["n"], c["kin"], c["ldx"], dtype)
    w = _v(c, c["w"], c["no"], c["ki"], c["ldw"], dtype)
    y = x @ w.t() if c["layout"] == NT else x @ w
    if c["bias"] is not None:
        y = y + _v(c, c["bias"], 1, c["kout"], c["kout"], dtype)
    return [_region(c["y"], c["n"], c["kout"], c["ldy"], y, "y")]


def small_form(c, base=lambda name: 0):
    """rows_small_kernel<VX, VY>."""
    def al16(ref):
        return (base(ref[0]) + 4 * ref[1]) % 16 == 0

    return (c["kin"] % 4 == 0 and c["ldx"] % 4 == 0 and al16(c["x"]), c["ldy"] % 4 == 0 and al16(c["y"]))


def small_rpb(kout):
    """Rows per workgroup: 256 >> tpr_log2, 4 * 2^tpr_log2 >= kout."""
    tl = 0
    while (1 << tl) * 4 < kout:
        tl += 1
    return 256 >> tl


def small_blocks(kin, kout, cus):
    """The launch's workgroup limit (persistent: per_cu per CU)."""
    lds = kin * ((kout + 3) & ~3) * 4
    return max(1, min(8, 131072 // lds)) * cus


SMALL_MAPS = [(1, 1), (128, 1), (128, 128), (4, 128), (5, 3), (16, 4), (17, 5), (62, 8), (4, 30), (16, 100),
              (62, 128), (128, 30), (17, 100), (1, 8), (16, 3)]
# (ldx_pad, xfront, ldy_pad, yfront): tight / padded strides, aligned / offset pointers
SMALL_FORMS = [(0, 4, 0, 4), (4, 4, 3, 4), (0, 5, 4, 4), (3, 4, 4, 5), (4, 4, 4, 4), (0, 4, 0, 5)]


def cases_d(cus):
    t = {}
    i = 0
    for lay in (NT, NN):
        for kin, kout in SMALL_MAPS:
            rpb = small_rpb(kout)
            n = (1, 7, rpb - 1, rpb + 1)[i % 4]
            f = SMALL_FORMS[i % 6]
            nm = f"small-{LAYOUT[lay]}-{kin}to{kout}-n{n}-f{i % 6}"
            t[nm] = functools.partial(small_case, nm, 500 + i, lay, kin, kout, n, bias=lay == NT and i % 2 == 0,
                                      ldx_pad=f[0], xfront=f[1], ldy_pad=f[2], yfront=f[3])
            i += 1
    # rows stride over the persistent workgroups (128 -> 128: the fewest rows that do)
    n = 2 * small_blocks(128, 128, cus) * small_rpb(128) + 5
    t["small-NT-128to128-strided"] = functools.partial(small_case, "small-NT-128to128-strided", 599, NT, 128, 128,
                                                       n, bias=True)
    return t


# --------------------------------------------------------------------------- ops.LinearRows
ROWS_E = (1, 31, 33, 127, 129)
MAPS_E = ((128, 128), (257, 128), (260, 300), (264, 20), (72, 40), (4, 128), (64, 30))


def linear_routes(k, nout):
    """The kernels ops.LinearRows reaches for y = x W^T (x [n, k], W [nout, k],
    n < 4096), from the predicates of rows.linear_fwd / linear_bwd_input /
    linear_bwd_weight: ("small",) or ("rgemm", kh, ns) per direction."""
    def rg(kk):
        kh, _, _, rest = rows._halves(torch.empty(0), torch.empty(0), kk)
        return ("rgemm", kh, rest)

    fwd = ("small",) if rows._skinny(k, nout) else rg(k)
    dx = ("small",) if k <= 128 and nout <= 128 and (min(k, nout) <= 16 or not rows._mfma_width(nout)) else rg(nout)
    return dict(fwd=fwd, dx=dx, dw=("tn",))


@functools.lru_cache(maxsize=None)
def linear_case(n, k, nout):
    g = torch.Generator().manual_seed(7000 + 1009 * n + 31 * k + nout)
    c = dict(x=torch.randn(n, k, generator=g), w=torch.randn(nout, k, generator=g) / k ** 0.5,
             b=torch.randn(nout, generator=g), dy=torch.randn(n, nout, generator=g))
    for dtype in (torch.float64, torch.float32):
        x, w, b = (c[q].to(dtype, copy=True).requires_grad_() for q in "xwb")
        y = torch.addmm(b, x, w.t())
        (y * c["dy"].to(dtype)).sum().backward()
        c[dtype] = dict(y=y.detach(), dx=x.grad, dw=w.grad, db=b.grad)
    c["bars"] = dict(y=1e-5 if k <= 260 else 2e-5, dx=1e-5 if nout <= 260 else 2e-5, dw=2e-5, db=2e-5)
    return c


# --------------------------------------------------------------------------- judging
REFERENCE = {"rgemm": rgemm_reference, "tn": tn_reference, "small": small_reference}


@functools.lru_cache(maxsize=8)
def build(group, name, cus):
    table = {"A": lambda: cases_a(cus), "B": cases_b, "C": cases_c, "D": lambda: cases_d(cus)}[group]()
    c = table[name]()
    assert c["name"] == name or name.endswith("-multi"), (c["name"], name)
    for flat in c["bufs"].values():
        assert flat.data_ptr() % 16 == 0
    return c


def reference(c, dtype=torch.float64):
    """The regions the call owns with their values; the float64 ones are computed once per case."""
    if dtype != torch.float64:
        return REFERENCE[c["kind"]](c, dtype)
    if "_ref64" not in c:
        c["_ref64"] = REFERENCE[c["kind"]](c, dtype)
    return c["_ref64"]


def owned(c, regions):
    """name -> bool mask of the floats of each output buffer the call owns."""
    m = {}
    for r in regions:
        name, o = r["ref"]
        own = m.setdefault(name, torch.zeros_like(c["bufs"][name], dtype=torch.bool))
        view(own, o, r["rows"], r["cols"], r["ld"]).fill_(True)
    return m


def judge(c, got, share=1.0):
    """got: name -> flat fp32 CPU tensor of every output buffer after the call.
    Asserts the bars (times share), the exact zeros, no NaN, and every float
    the call does not own bitwise as it was.  Returns the largest error as a
    share of its scale."""
    regions = reference(c)
    for name, own in owned(c, regions).items():
        before, after = c["bufs"][name], got[name]
        assert torch.equal(after[~own].view(torch.int32), before[~own].view(torch.int32)), \
            (c["name"], name, "a float outside the output was written")
    scales = {}
    for r in regions:
        s = r["scale"] if r["scale"] is not None else r["values"].abs().max().item()
        scales[r["grp"]] = max(scales.get(r["grp"], 0.0), s)
    worst = 0.0
    for r in regions:
        y = view(got[r["ref"][0]], r["ref"][1], r["rows"], r["cols"], r["ld"])
        assert not torch.isnan(y).any(), (c["name"], r["grp"], "NaN let through")
        scale = scales[r["grp"]]
        err = (y.double() - r["values"]).abs().max().item()
        if scale == 0.0:
            assert err == 0.0 and not (y != 0).any(), (c["name"], r["grp"], "not an exact zero", err)
            continue
        assert math.isfinite(scale)
        print(f"{c['name']} {r['grp']}: max|err| {err:.3e} max|ref| {scale:.3e} ({err / scale:.2e})")
        assert err <= share * c["bar"] * scale, (c["name"], r["grp"], err, scale, err / scale)
        worst = max(worst, err / scale)
    return worst


def evaluate_fp32(c):
    """The outputs as torch float32 arithmetic on the CPU gives them."""
    got = {name: c["bufs"][name].clone() for name in owned(c, reference(c))}
    for r in reference(c, torch.float32):
        view(got[r["ref"][0]], r["ref"][1], r["rows"], r["cols"], r["ld"]).copy_(r["values"])
    return got
