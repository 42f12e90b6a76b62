"""Form table of the small dense kernel: the smallest shapes that land on every form of small_gemm_kernel<NW, AV, BV> (csrc/linear.hip)
through each of its three entry points, and on the edges inside a form.

NW waves (1, 2, 4, 8, 16) split K and combine through LDS; AV / BV read the operand 16 bytes per lane.  Which of the 20 a launch takes
is decided by K, the tile count, the strides, the z strides, every entry of the offset table and the alignment of the two base pointers;
te_small_gemm_form (include/te_hip.h) reports the plan that the launch itself makes and then dispatches on.  An entry names the entry
point, the dims, nz (S for the split-K form), how A and B lie in memory, the epilogue, and the form key (nw, av, bv) it is expected to
land on.  The expected key is data; what a launch does comes from the query.  tests/test_small_gemm_forms_cpu.py checks the table
against the query and sweeps the query for keys the table lacks; tests/test_gpu_small_gemm_forms.py runs every entry against fp64
after re-asserting its key.  The list of keys with their entries: `python tests/small_gemm_forms.py`.

Entry points (ep): 'single' te_small_gemm_f32, 'uniform' te_small_gemm_batched_f32 with zb / zbias, 'table' the same with b_tab /
bias_tab, 'splitk' te_small_gemm_splitk_f32 (K is the whole reduction, nz = S chunks of Kc = K / S; the key is that of the chunk launch).

Layouts of an operand with R rows (I for A, J for B) and reduction length K, as (row stride, reduction stride, base offset), LAYOUTS:
    dense    (K, 1, 0)          unit reduction stride, 16-byte aligned base; 16-byte loads when K % 4 == 0
    off4     (K, 1, 1)          the same at a base 4 bytes off 16-byte alignment: scalar loads
    oddrow   (K + 1 | 2, 1, 0)  unit reduction stride, row stride % 4 != 0: scalar loads
    padded   (K4 + 8, 1, 0)     a row slice of a wider tensor, row stride % 4 == 0: 16-byte loads, with the scalar tail when K % 4 != 0
    trans    (1, R, 0)          transposed: reduction stride = row count
    every2   (2 K, 2, 0)        both strides > 1: every other element of a [R, 2 K] tensor
In a batched launch slice z of A starts za = (the slice's extent rounded up to 4) after slice z - 1 (za_mode 'sep'), one element more
('odd': za % 4 == 1, AV off) or at the same place ('zero': a shared input).  B slices lie zb apart (uniform) or in reverse order at
b_tab (table; tab_odd = t moves slice t one element on, so that b_tab[t] % 4 == 1 and BV is off).  C is dense [nz, I, J] ('dense') or
lies in a [I, nz + 1, J] ('btd') or [I, J, nz + 1] ('bdt') buffer, whose last token no launch writes.

K edges.  A wave's range is kq = ceil(K / 8 NW) * 8 wide; with K % 4 != 0 on a 16-byte form the last wave that has work runs the float4
path and the scalar tail in the same loop (lane half 1 starts 4 past half 0).  Per (NW, K): which waves are short or empty
    NW 1   K 1: one element, tail only    5: half 0 float4, half 1 one tail element    8: one full step    16: two full steps
    NW 2   K 17: wave 1 has one element    18: wave 1 has two    33: kq 24, wave 1 has 9    64: both full
    NW 4   K 65: kq 24, wave 2 has 17, wave 3 empty    100: kq 32, wave 3 has 4    256: all full
    NW 8   K 257: kq 40, wave 6 has 17, wave 7 empty    300: kq 40, wave 7 has 20    511: kq 64, wave 7 has 63
    NW 16  K 513: kq 40, wave 12 has 33, waves 13-15 empty    520: waves 13-15 empty    1000: kq 64, wave 15 has 40    1024: all full

Epilogue of an entry: alpha (None: 1 / sqrt(K)), bias with beta, act (0 none, 1 GELU, 3 leaky ReLU * sqrt 2), pre wanted, residual,
rs = rs_scale of the row sums (None: not wanted).  Every act = 3 entry has a bias of magnitude >= 3 with beta = 1 and alpha = 1 / sqrt(K),
which keeps its pre-activations off the kink (reference() below, checked on the CPU for every such entry).

reference() is the fp64 restatement and the elementwise bound of the GPU test; it runs on whatever device the operands are on.
"""
import dataclasses
import math
import os
import sys
from dataclasses import dataclass

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from fp64_check import A32, KINK_CAP, S32, U32 as U, kink_keep, where64  # noqa: E402  (slope and gain as the kernel has them)
from transeditor_amd import _lib  # noqa: E402

LAYOUTS = ('dense', 'off4', 'oddrow', 'padded', 'trans', 'every2')
EPS = ('single', 'uniform', 'table', 'splitk')
TAIL = 64                                          # spare elements behind every operand


@dataclass(frozen=True)
class Entry:
    name: str
    ep: str
    I: int
    J: int
    K: int
    nz: int              # 1 for 'single', S for 'splitk'
    la: str
    lb: str
    key: tuple           # (nw, av, bv)
    bias: int = 0
    alpha: float = None  # None: 1 / sqrt(K)
    beta: float = 1.0
    act: int = 0
    pre: int = 0
    res: int = 0
    rs: float = None
    za_mode: str = 'sep'
    tab_odd: int = -1
    cl: str = 'dense'

    def __hash__(self):
        return hash(self.name)


TABLE = []


def E(tag, ep, I, J, K, nz, la, lb, key, **kw):
    if kw.get('act') == 3:
        kw.setdefault('bias', 1)
    name = f'{ep}_nw{key[0]}_a{key[1]}b{key[2]}_{I}x{J}x{K}' + (f'_z{nz}' if ep != 'single' else '') + f'_{tag}'
    same = sum(t.name == name or t.name.startswith(name + '#') for t in TABLE)
    e = Entry(name + (f'#{same + 1}' if same else ''), ep, I, J, K, nz, la, lb, tuple(key), **kw)
    TABLE.append(e)
    return e


# ---- every (entry point, key): K per NW, dense or transposed per AV / BV.  K = 512 on 3 x 2 tiles is the first way to 16 waves.
ACTS = (dict(act=0), dict(act=1, pre=1), dict(act=3, pre=1), dict(act=3, res=1), dict(act=1, bias=1, beta=0.75), dict(act=0, bias=1, beta=-1.5, res=1))
n = 0
for nw, K in ((1, 12), (2, 40), (4, 96), (8, 300), (16, 512)):
    for la, av in (('dense', 1), ('trans', 0)):
        for lb, bv in (('dense', 1), ('trans', 0)):
            E('form', 'single', 33, 65, K, 1, la, lb, (nw, av, bv), **ACTS[n % 6])
            E('form', 'uniform', 5, 33, K, 3, la, lb, (nw, av, bv), **{k: v for k, v in ACTS[(n + 1) % 6].items() if k in ('act', 'bias', 'beta')})
            n += 1
for nw, K in ((1, 12), (2, 40), (4, 96), (8, 300), (16, 516)):
    for la, av in (('dense', 1), ('every2', 0)):
        # BV off by the layout, and by a single table entry with offset % 4 != 0 under a layout that would allow it
        E('form', 'table', 5, 33, K, 3, la, 'dense', (nw, av, 1), bias=1, beta=0.75)
        E('form', 'table', 5, 33, K, 3, la, 'trans', (nw, av, 0), act=3)
        E('tabodd', 'table', 5, 33, K, 3, la, 'dense', (nw, av, 0), tab_odd=1, bias=nw in (2, 8), beta=0.75)
for nw, Kc in ((1, 8), (2, 24), (4, 96), (8, 304), (16, 520)):
    for la, av in (('dense', 1), ('trans', 0)):
        for lb, bv in (('dense', 1), ('every2', 0)):
            E('form', 'splitk', 5, 40, 2 * Kc, 2, la, lb, (nw, av, bv), **ACTS[n % 6])
            n += 1

# ---- the other ways to 8 and 16 waves.  K = 512 needs 2 * kNumCU = 512 tiles for 8 waves: 23 x 23 tiles is the squarest grid with
# that many (I = J = 705); one tile row fewer (22 x 23 = 506) is back at 16.  These two are the large single launches.
E('tiles529', 'single', 705, 705, 512, 1, 'dense', 'dense', (8, 1, 1), act=3, pre=1)
E('tiles506', 'single', 673, 705, 512, 1, 'dense', 'dense', (16, 1, 1))
E('tiles516', 'uniform', 33, 65, 512, 86, 'dense', 'dense', (8, 1, 1), za_mode='zero', bias=1)
E('k513', 'single', 33, 65, 513, 1, 'padded', 'padded', (16, 1, 1), act=3, pre=1, res=1)
E('k1024', 'single', 33, 65, 1024, 1, 'dense', 'dense', (16, 1, 1), act=3, pre=1)

# ---- K edges per NW (see the docstring for the waves): on the 16-byte form (padded rows where K % 4 != 0, so that float4 path and
# scalar tail run in one wave) and on the scalar form
for nw, Ks in ((1, (1, 5, 8, 16)), (2, (17, 18, 33, 64)), (4, (65, 100, 256)), (8, (257, 300, 511)), (16, (513, 520, 1000, 1024))):
    for K in Ks:
        lay = 'padded' if K % 4 else 'dense'
        E('kedge', 'single', 37, 33, K, 1, lay, lay, (nw, 1, 1), rs=0.37, bias=1, beta=0.75, pre=1, act=1)
        E('kedge', 'single', 37, 33, K, 1, 'trans', 'oddrow' if K > 1 else 'trans', (nw, 0, 0), rs=-1.25, act=3, pre=1)

# ---- tile edges at K = 24 (two waves): every I, J of {1, 31, 32, 33, 65}
for i, I in enumerate((1, 31, 32, 33, 65)):
    for j, J in enumerate((1, 31, 32, 33, 65)):
        E('tile', 'single', I, J, 24, 1, 'dense', 'dense' if (i + j) % 2 else 'trans', (2, 1, (i + j) % 2), rs=0.5, **ACTS[(i + 2 * j) % 6])
E('tile', 'single', 1, 1, 16, 1, 'dense', 'dense', (1, 1, 1), act=3)
E('tile', 'single', 31, 33, 17, 1, 'padded', 'padded', (2, 1, 1), act=3, pre=1)
E('tile', 'single', 65, 33, 300, 1, 'dense', 'dense', (8, 1, 1), act=3, res=1)
E('tile', 'single', 7, 40, 96, 1, 'dense', 'dense', (4, 1, 1), act=3, pre=1, res=1)

# ---- operand layouts, A and B separately (K = 96; K = 99 for the ones whose form does not depend on K % 4)
for lay, v in (('dense', 1), ('off4', 0), ('oddrow', 0), ('padded', 1), ('trans', 0), ('every2', 0)):
    E('layA', 'single', 33, 40, 96, 1, lay, 'dense', (4, v, 1), rs=0.37, bias=1, beta=0.75)
    E('layB', 'single', 33, 40, 96, 1, 'dense', lay, (4, 1, v), rs=0.37, act=1, pre=1)
    E('layAB', 'single', 33, 40, 99, 1, lay, lay, (4, int(lay == 'padded'), int(lay == 'padded')), rs=0.37, act=3, pre=1)
E('layAB', 'single', 33, 40, 516, 1, 'off4', 'off4', (16, 0, 0), rs=0.37)
E('layAB', 'single', 33, 40, 516, 1, 'dense', 'dense', (16, 1, 1), rs=0.37)

# ---- epilogue on one shape: bias on / off with beta != 1, alpha != 1, every act, pre wanted or not, residual on or off
for act in (0, 1, 3):
    for pre in (0, 1):
        for res in (0, 1):
            E('epi', 'single', 7, 40, 96, 1, 'dense', 'dense', (4, 1, 1), act=act, pre=pre, res=res, bias=int(act == 3 or pre != res),
              beta=1.0 if act == 3 else -0.6, alpha=None if act == 3 else (1.0, -0.3)[res])
# row sums with rs_scale != 1 at J = 1, 33, 65 and ragged I; with more than one column block only block column 0 may write
for J in (1, 33, 65):
    E('rowsum', 'single', 37, J, 5, 1, 'trans', 'dense', (1, 0, 0), rs=0.37)
    E('rowsum', 'single', 37, J, 100, 1, 'padded', 'trans', (4, 1, 0), rs=-2.5, act=1)
    E('rowsum', 'single', 70, J, 513, 1, 'trans', 'padded', (16, 0, 1), rs=1.0 / 3)

# ---- batched: nz 1, 3, 16; uniform and table; C written into the [B, tokens, D] and [B, D, tokens] layouts of a larger buffer
for nz in (1, 3, 16):
    for cl in ('dense', 'btd', 'bdt'):
        E(cl, 'uniform', 5, 33, 40, nz, 'dense', 'dense', (2, 1, 1), cl=cl, act=3)
        E(cl, 'table', 5, 33, 40, nz, 'dense', 'dense', (2, 1, 1), cl=cl, bias=int(cl != 'btd'), beta=0.75, act=int(cl == 'bdt'))
    E('tabodd', 'table', 5, 33, 40, nz, 'dense', 'dense', (2, 1, 0), tab_odd=nz - 1, act=3, cl='btd')
    E('zaodd', 'uniform', 5, 33, 40, nz, 'dense', 'dense', (2, 0, 1), za_mode='odd', bias=1, beta=0.75)      # (the plan reads za at nz = 1 too)
    E('zazero', 'uniform', 33, 5, 40, nz, 'padded', 'trans', (2, 1, 0), za_mode='zero', act=1, cl='bdt')
E('zaodd', 'table', 5, 33, 100, 3, 'padded', 'padded', (4, 0, 1), za_mode='odd', act=3, cl='bdt')

# ---- split-K: S 1, 2, 3, 8 with Kc 8, 768, 1024 on ragged I * J, act 1 and 3 with pre, bias and residual; and the two shapes the model has
n = 0
for S in (1, 2, 3, 8):
    for Kc, nw in ((8, 1), (768, 16), (1024, 16)):
        E('chunks', 'splitk', 5, 40, S * Kc, S, 'dense', 'dense', (nw, 1, 1), act=(1, 3)[n % 2], pre=1, bias=1, res=1, beta=1.0 if n % 2 else 0.75)
        n += 1
E('disc', 'splitk', 32, 512, 8192, 8, 'dense', 'dense', (16, 1, 1), act=3, pre=1)
E('case', 'splitk', 5, 40, 2304, 3, 'dense', 'dense', (16, 1, 1), act=3, pre=1, res=1)
del n

BY_NAME = {e.name: e for e in TABLE}
assert len(BY_NAME) == len(TABLE), 'entry names must be unique'
LARGE = ('single_nw8_a1b1_705x705x512_tiles529', 'single_nw16_a1b1_673x705x512_tiles506', 'splitk_nw16_a1b1_32x512x8192_z8_disc',
         'splitk_nw16_a1b1_5x40x2304_z3_case')


# ------------------------------------------------------------------------------------------------ where the operands lie
def layout(name, R, K):
    """(row stride, reduction stride, base offset) of an R x K operand"""
    if name == 'dense':
        return K, 1, 0
    if name == 'off4':
        return K, 1, 1
    if name == 'oddrow':
        return (K + 1 if (K + 1) % 4 else K + 2), 1, 0
    if name == 'padded':
        return -(-K // 4) * 4 + 8, 1, 0
    if name == 'trans':
        return 1, R, 0
    if name == 'every2':
        return 2 * K, 2, 0
    raise ValueError(name)


def _up4(n):
    return -(-n // 4) * 4


@dataclass(frozen=True)
class Geom:
    """the arguments of an entry's launch, in elements; a_off / b_off: the base inside its storage tensor of a_numel / b_numel elements"""
    sai: int
    sak: int
    a_off: int
    za: int
    a_numel: int
    sbk: int
    sbj: int
    b_off: int
    zb: int
    b_tab: tuple          # None but for 'table'
    b_starts: tuple       # offset of slice z from the base of B
    b_numel: int
    zbias: int
    bias_tab: tuple
    bias_starts: tuple
    zc: int
    sci: int
    scj: int
    c_numel: int


def geom(e):
    nz = 1 if e.ep in ('single', 'splitk') else e.nz
    sai, sak, a_off = layout(e.la, e.I, e.K)
    sbj, sbk, b_off = layout(e.lb, e.J, e.K)
    a_span = (e.I - 1) * sai + (e.K - 1) * sak + 1
    b_span = (e.J - 1) * sbj + (e.K - 1) * sbk + 1
    za = {'sep': _up4(a_span), 'odd': _up4(a_span) + 1, 'zero': 0}[e.za_mode]
    slot = _up4(b_span) + 4
    b_tab = bias_tab = None
    if e.ep == 'table':
        b_tab = tuple((nz - 1 - z) * slot + (1 if z == e.tab_odd else 0) for z in range(nz))
        bias_tab = tuple((nz - 1 - z) * e.J for z in range(nz))
        zb = zbias = 0
        b_starts, bias_starts = b_tab, bias_tab
    else:
        zb, zbias = slot, e.J
        b_starts, bias_starts = tuple(z * zb for z in range(nz)), tuple(z * zbias for z in range(nz))
    if e.cl == 'btd':
        zc, sci, scj, c_numel = e.J, (nz + 1) * e.J, 1, e.I * (nz + 1) * e.J
    elif e.cl == 'bdt':
        zc, sci, scj, c_numel = 1, e.J * (nz + 1), nz + 1, e.I * e.J * (nz + 1)
    else:
        zc, sci, scj, c_numel = e.I * e.J, e.J, 1, nz * e.I * e.J
    return Geom(sai, sak, a_off, za, a_off + (nz - 1) * za + a_span + TAIL, sbk, sbj, b_off, zb, b_tab, b_starts,
                b_off + nz * slot + TAIL, zbias, bias_tab, bias_starts, zc, sci, scj, c_numel)


def answer(e, g=None):
    """te_small_gemm_form's answer (nw, av, bv, grid x, y, z) for an entry; a negative TE_ERR_* code where the launch refuses"""
    g = g or geom(e)
    if e.ep == 'splitk':
        return _lib.small_gemm_form(e.I, e.J, e.K, e.nz, g.sai, g.sak, g.sbk, g.sbj, a_mod16=4 * g.a_off % 16, b_mod16=4 * g.b_off % 16, splitk=True)
    return _lib.small_gemm_form(e.I, e.J, e.K, e.nz, g.sai, g.sak, g.sbk, g.sbj, g.za, g.zb, g.b_tab, 4 * g.a_off % 16, 4 * g.b_off % 16)


def check(e):
    """raise AssertionError naming the entry when the library does not plan the declared key for it; returns the answer"""
    ans = answer(e)
    assert not isinstance(ans, int), f'{e.name}: te_small_gemm_form refuses ({ans})'
    assert ans[:3] == e.key, f'{e.name}: expected (nw, av, bv) = {e.key}, the library plans {ans[:3]}'
    nz = e.nz if e.ep != 'single' else 1
    assert ans[3:] == (-(-e.J // 32), -(-e.I // 32), nz), f'{e.name}: grid {ans[3:]}'
    return ans


# ------------------------------------------------------------------------------------------------ operands and the fp64 reference
FILL = 3.0                  # what lies between the addressed elements of an operand


def _f32(v):
    return float(np.float32(v))


def scalars(e):
    """(alpha, beta, rs_scale) as the fp32 values the launch receives"""
    return _f32(1.0 / math.sqrt(e.K) if e.alpha is None else e.alpha), _f32(e.beta), (None if e.rs is None else _f32(e.rs))


def operands(e, seed=None, device='cpu', g=None):
    """the entry's tensors from a CPU generator seeded by the entry's place in the table: the storage tensors 'a', 'b' (the launch's base
    pointers are a[a_off:], b[b_off:]), 'bias' [nz * J] or None, 'res' [I, J] or None.  The VALUES depend on the seed and the dims only,
    not on the layouts: two entries that differ in layout alone hold the same matrices."""
    g = g or geom(e)
    nz = 1 if e.ep in ('single', 'splitk') else e.nz
    gen = torch.Generator().manual_seed(2000 + TABLE.index(e) if seed is None else seed)
    rn = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float32)
    A, B, bn = rn(1 if e.za_mode == 'zero' else nz, e.I, e.K), rn(nz, e.J, e.K), rn(nz, e.J)
    res = rn(e.I, e.J)
    a = torch.full((g.a_numel,), FILL)
    b = torch.full((g.b_numel,), FILL)
    for z in range(A.shape[0]):
        a.as_strided((e.I, e.K), (g.sai, g.sak), g.a_off + z * g.za).copy_(A[z])
    for z in range(nz):
        b.as_strided((e.J, e.K), (g.sbj, g.sbk), g.b_off + g.b_starts[z]).copy_(B[z])
    bias = None
    if e.bias:
        bias = torch.empty(nz * e.J)
        for z in range(nz):
            bias[g.bias_starts[z]:g.bias_starts[z] + e.J] = torch.sign(bn[z]) * (3.0 + 0.5 * bn[z].abs())
    o = {'a': a, 'b': b, 'bias': bias, 'res': res if e.res else None}
    return {k: (v.to(device) if v is not None else None) for k, v in o.items()}


def views64(e, o, g=None):
    """(A [nz, I, K], B [nz, J, K], bias [nz, J] | None) in fp64, taken through as_strided with the very strides handed to the kernel"""
    g = g or geom(e)
    nz = 1 if e.ep in ('single', 'splitk') else e.nz
    a, b = o['a'].double(), o['b'].double()
    A = a.as_strided((nz, e.I, e.K), (g.za, g.sai, g.sak), g.a_off)
    B = torch.stack([b.as_strided((e.J, e.K), (g.sbj, g.sbk), g.b_off + g.b_starts[z]) for z in range(nz)])
    bias = None if o['bias'] is None else torch.stack([o['bias'].double()[s:s + e.J] for s in g.bias_starts])
    return A, B, bias


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def gelu_term(pre):
    """bound of the fp32 GELU at a given fp32 argument: three product roundings and one add on the result, erf to 16 ulp, one more ulp
    for the rounded argument of erf (|t erf'(t)| < 0.5)"""
    return 4 * U * gelu64(pre).abs() + 0.5 * pre.abs() * (16 + 1) * U


def reference(e, o, nw, g=None):
    """fp64 reference and elementwise bounds of an entry, all [nz, I, J] ([nz, I] for the row sums), as a dict:
    pre, pre_bound, out, out_bound (act = 1: for a launch that does not hand out pre), keep (None unless act = 3), rs, rs_bound"""
    g = g or geom(e)
    alpha, beta, rs = scalars(e)
    A, B, bias = views64(e, o, g)
    acc = torch.matmul(A, B.transpose(1, 2))
    P = torch.matmul(A.abs(), B.abs().transpose(1, 2)) * abs(alpha)
    bb = torch.zeros_like(acc) if bias is None else (beta * bias)[:, None, :].expand_as(acc)
    pre = alpha * acc + bb
    if e.ep == 'splitk':         # S partial sums of Kc products on nw waves, their sum in the second kernel, then alpha
        L = e.K // e.nz + nw + e.nz + 1
    else:
        L = e.K + nw + 1
    pre_bound = L * U * P + U * bb.abs() + U * pre.abs()
    r = {'pre': pre, 'pre_bound': pre_bound, 'keep': None, 'L': L}
    if e.act == 3:
        slope = where64(pre > 0, S32, A32 * S32)
        out = pre * slope
        bound = pre_bound * slope + 2 * U * out.abs()
        r['keep'] = kink_keep(pre, pre_bound)
    elif e.act == 1:
        out = gelu64(pre)
        bound = 1.13 * pre_bound + gelu_term(pre)
    else:
        out, bound = pre, pre_bound
    if o['res'] is not None:
        out = out + o['res'].double()
        bound = bound + U * out.abs()
    r['out'], r['out_bound'] = out, bound
    if rs is not None:
        r['rs'] = rs * A.sum(2)
        r['rs_bound'] = (e.K + 2 * nw + 1) * U * abs(rs) * A.abs().sum(2)
    return r


def left_out(e, r):
    """share of the entry's outputs that the kink leaves out; entries with fewer than 1000 outputs may leave out none"""
    return 0.0 if r['keep'] is None else 1.0 - float(r['keep'].double().mean())


def kink_ok(e, r):
    left = left_out(e, r)
    return left == 0.0 if r['pre'].numel() < 1000 else left <= KINK_CAP


if __name__ == '__main__':
    by_key = {}
    for e in TABLE:
        by_key.setdefault((e.ep,) + e.key, []).append(e.name)
    for k in sorted(by_key):
        print(k, ':', ', '.join(by_key[k]))
    print(f'{len(by_key)} (entry point, key) pairs, {len(TABLE)} entries')
