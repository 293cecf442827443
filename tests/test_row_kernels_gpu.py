"""The three row-wise streaming kernels through the C ABI -- ``ver_add_ln_*`` and ``ver_relu_dropout_*`` (csrc/ver_addln.hip),
``ver_ln_relu_*`` (csrc/ver_mlp.hip) -- against the exact fp64 chain, under bounds formed from the references alone
(row_kernels_helper: 4 d_ref + 16 ulps), at every width, at the launchers' grid-stride edges, with the dropout mask pinned to
``hipops.dropout_keep_host`` for seeds the tests own, on edge rows, into NaN-filled buffers with a guard band behind them.
test_row_kernels_cpu.py plants the faults these bounds exist for.  Every comparison prints d_ref, the kernel's distance and
the bound (docs/HISTORY.md records the three grid-stride cases)."""
import pytest
import torch

import row_kernels_helper as H
from util import pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
GARBAGE = 12345.0
# Row counts from the launchers' constants: ver_add_ln_forward caps its grid at 8 192 workgroups of 4 rows, the backward at
# 2 048; 32 768 + 5 rows take the forward's second trip and the backward's fifth, 8 192 + 5 the backward's second, all ragged.
ADD_LN_TWO_TRIPS = H.ADD_LN_FWD_GRID * H.ADD_LN_ROWS + 5
ADD_LN_BWD_TWO_TRIPS = H.ADD_LN_BWD_GRID * H.ADD_LN_ROWS + 5
# ver_relu_dropout_*: 16 384 workgroups x 256 threads x 4 elements a trip; the second with a ragged tail
RELU_DROPOUT_TWO_TRIPS = H.RELU_DROPOUT_GRID * H.RELU_DROPOUT_PER_WG + 1028
# ver_ln_relu_*: 4 096 workgroups of 16 rows
LN_RELU_TWO_TRIPS = H.LN_RELU_GRID * H.LN_RELU_ROWS + 17
assert (ADD_LN_TWO_TRIPS, ADD_LN_BWD_TWO_TRIPS, RELU_DROPOUT_TWO_TRIPS, LN_RELU_TWO_TRIPS) == (32773, 8197, 16778244, 65553)


def _code(dtype):
    return 1 if dtype == BF16 else 0


def _nan(count, dtype=F32):
    return torch.full((count,), float('nan'), dtype=dtype, device=DEV)


def _untouched(buf, used):
    """the guard band behind the first ``used`` elements still holds the fill, bit for bit"""
    ity = torch.int32 if buf.dtype == F32 else torch.int16
    tail = buf[used:]
    return tail.numel() > 0 and torch.equal(tail.view(ity), torch.full_like(tail, float('nan')).view(ity))


def _call(lib, fn, *args):
    rc = fn(*args)
    assert rc == 0, lib.ver_last_error()


def _refused(lib, rc, text):
    msg = lib.ver_last_error().decode()
    assert rc != 0 and text in msg, (rc, msg)


def _check(title, r, got):
    d = H.measure(r, got)
    print(H.table(title, r['d_ref'], d, r['bound']))
    for k in r['exact']:
        assert k in d, k                                   # everything the reference holds was compared
    bad = H.violations(d, r['bound'])
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------ add_ln
def _add_ln(hip, inp, p_drop, seed, use_gy16=True, finite=True):
    """One forward and one backward call into NaN-filled buffers with a guard row behind row N; the parameter gradients start
    as garbage.  Returns the outputs on the CPU."""
    lib, p, st = hip.lib(), hip._p, hip._stream()
    n, c = inp['res'].shape
    adt = inp['a'].dtype
    a, res, g, b, gy = (inp[k].to(DEV).contiguous() for k in ('a', 'res', 'gamma', 'beta', 'gy'))
    gy16 = inp['gy16'].to(DEV).contiguous() if use_gy16 else None
    sd = torch.tensor([seed], dtype=torch.int64, device=DEV) if p_drop > 0 else None      # (p = 0: the seed may be NULL)
    rows = (n + 1) * c
    y, y16, mean, rstd = _nan(rows), _nan(rows, BF16), _nan(n + 1), _nan(n + 1)
    _call(lib, lib.ver_add_ln_forward, p(a), _code(adt), p(res), p(g), p(b), p(sd), p_drop, H.EPS, p(y), p(y16), p(mean),
          p(rstd), n, c, st)
    d_a, d_res = _nan(rows, adt), _nan(rows)
    dg, db = torch.full((c,), GARBAGE, device=DEV), torch.full((c,), -GARBAGE, device=DEV)
    _call(lib, lib.ver_add_ln_backward, p(gy), p(gy16), p(a), _code(adt), p(res), p(g), p(mean), p(rstd), p(sd), p_drop,
          p(d_a), p(d_res), p(dg), p(db), n, c, st)
    torch.cuda.synchronize()
    for name, buf, used in (('y', y, n * c), ('y_bf16', y16, n * c), ('mean', mean, n), ('rstd', rstd, n),
                            ('d_a', d_a, n * c), ('d_res', d_res, n * c)):
        assert _untouched(buf, used), 'guard band of %s' % name
        if finite:
            assert bool(torch.isfinite(buf[:used].float()).all()), '%s was not written in full' % name
    if finite:
        assert bool(torch.isfinite(dg).all()) and bool(torch.isfinite(db).all())
    return dict(y=y[:n * c].view(n, c).cpu(), y16=y16[:n * c].view(n, c).cpu(), mean=mean[:n].cpu(), rstd=rstd[:n].cpu(),
                d_a=d_a[:n * c].view(n, c).cpu(), d_res=d_res[:n * c].view(n, c).cpu(), d_gamma=dg.cpu(), d_beta=db.cpu())


def _add_ln_case(n, c, adt, p_drop, seed, use_gy16=True, edge=False, twice=False):
    hip = pkg('hipops')
    r = H.add_ln_reference(n, c, adt, p_drop, seed, use_gy16, edge)
    got = _add_ln(hip, r['inp'], p_drop, seed, use_gy16)
    assert torch.equal(got['y16'].view(torch.int16), got['y'].bfloat16().view(torch.int16))      # bit for bit
    assert got['d_a'].dtype == adt
    assert bool((got['d_a'][~r['keep']] == 0).all())       # dropped by the host rule: exactly 0, no element excused
    _check('add_ln n=%d C=%d a=%s p=%g seed=%d gy16=%d' % (n, c, str(adt)[6:], p_drop, seed, use_gy16), r, got)
    if twice:                                              # (d(gamma) / d(beta): float atomics across workgroups, no such claim)
        again = _add_ln(hip, r['inp'], p_drop, seed, use_gy16)
        for k in ('y', 'y16', 'mean', 'rstd', 'd_a', 'd_res'):
            assert torch.equal(got[k], again[k]), k
    return r, got


@pytest.mark.parametrize('use_gy16', [True, False])
@pytest.mark.parametrize('p_drop', [0.0, 0.1])
@pytest.mark.parametrize('adt', DTYPES)
@pytest.mark.parametrize('c', [256, 512, 768, 1024])
def test_add_ln_every_width(c, adt, p_drop, use_gy16):
    """every instantiation k_add_ln_*<ABF16, K> (C = 512 is K = 2), 5 rows: two workgroups, the last with one live wave of
    four; grad_y alone and grad_y + grad_y_bf16."""
    _add_ln_case(5, c, adt, p_drop, 1, use_gy16)


@pytest.mark.parametrize('n,c,adt', [(1, 256, F32), (1, 256, BF16), (4, 256, F32), (4, 256, BF16),
                                      (ADD_LN_TWO_TRIPS, 256, F32), (ADD_LN_TWO_TRIPS, 256, BF16),
                                      (ADD_LN_BWD_TWO_TRIPS, 768, BF16)])
def test_add_ln_launch_edges(n, c, adt):
    """one row, one full workgroup, and the later trips of both grid-stride loops (row counts: top of the file); 8 197 rows of
    768 bf16 channels is the training step's instantiation on the backward's second trip.  Forward, d(a) and d(residual) are
    bit-identical over two runs."""
    _add_ln_case(n, c, adt, 0.1, 2 ** 62 - 1, twice=True)


@pytest.mark.parametrize('seed', H.SEEDS)
@pytest.mark.parametrize('adt', DTYPES)
def test_add_ln_mask_is_the_host_rule_for_every_seed(adt, seed):
    r, _ = _add_ln_case(5, 256, adt, 0.1, seed)
    assert 0 < int((~r['keep']).sum()) < r['keep'].numel()


@pytest.mark.parametrize('p_drop', [0.5, 0.999, 1e-8])
@pytest.mark.parametrize('adt', DTYPES)
def test_add_ln_dropout_probabilities(adt, p_drop):
    r, _ = _add_ln_case(5, 256, adt, p_drop, 1)
    if p_drop == 1e-8:                                     # 1.0f - 1e-8f == 1.0f: the fp32 threshold keeps everything
        assert bool(r['keep'].all())
    else:
        assert 0 < int(r['keep'].sum()) < r['keep'].numel()


@pytest.mark.parametrize('c', [256, 768])
@pytest.mark.parametrize('adt', DTYPES)
def test_add_ln_edge_rows(adt, c):
    """rows 1 (a = 0, residual = 4) and 3 (all zero): y == beta bit for bit and 1/std = 1/sqrt(eps); rows 2 and 40 of mean 100
    (where a one-pass variance is 7e-3 off); row 4 with magnitudes up to 1e15; all inside the bounds, gradients included."""
    r, got = _add_ln_case(H.EDGE_ROWS, c, adt, 0.1, 1, edge=True, twice=True)
    for row in (1, 3):
        assert torch.equal(got['y'][row].view(torch.int32), r['inp']['beta'].view(torch.int32))
        assert got['mean'][row] == r['inp']['res'][row, 0]
        assert abs(float(got['rstd'][row]) * H.EPS ** 0.5 - 1.0) <= r['bound'][('rstd', 'relmax')]


def test_add_ln_backward_of_no_rows_zeroes_the_parameter_gradients():
    hip = pkg('hipops')
    lib, p = hip.lib(), hip._p
    for c in (256, 768):
        dg, db = torch.full((c,), GARBAGE, device=DEV), torch.full((c,), -GARBAGE, device=DEV)
        _call(lib, lib.ver_add_ln_backward, None, None, None, 1, None, None, None, None, None, 0.1, None, None, p(dg), p(db),
              0, c, hip._stream())
        torch.cuda.synchronize()
        assert bool((dg == 0).all()) and bool((db == 0).all())


@pytest.mark.parametrize('adt', DTYPES)
def test_add_ln_non_finite_inputs(adt):
    """The contract include/ver_ops.h states: a NaN in residual (row 2) or in a KEPT element of a (row 4) makes its own row
    NaN -- y, mean, rstd, d(a), d(residual) -- and all of d(gamma); a NaN in a DROPPED element of a (row 6) contributes 0
    (torch's dropout would propagate it); every other row is bit-identical to the run without them."""
    hip = pkg('hipops')
    n, c, p_drop, seed = 9, 256, 0.5, 1
    r = H.add_ln_reference(n, c, adt, p_drop, seed)
    keep = r['keep']
    base = _add_ln(hip, r['inp'], p_drop, seed)
    inp = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in r['inp'].items()}
    kept, dropped = int(keep[4].nonzero()[3]), int((~keep[6]).nonzero()[3])
    inp['res'][2, 7] = float('nan')
    inp['a'][4, kept] = float('nan')
    inp['a'][6, dropped] = float('nan')
    got = _add_ln(hip, inp, p_drop, seed, finite=False)
    rows = torch.tensor([i not in (2, 4) for i in range(n)])
    for k in ('y', 'y16', 'd_res', 'mean', 'rstd'):
        assert bool(torch.isnan(got[k][~rows].float()).all()), k
    assert bool(torch.isnan(got['d_a'][~rows].float()[keep[~rows]]).all())
    assert bool((got['d_a'][~keep] == 0).all())            # a dropped element's gradient is 0 in a NaN row too
    for k in ('y', 'y16', 'd_a', 'd_res', 'mean', 'rstd'):
        assert torch.equal(got[k][rows], base[k][rows]), k
    assert bool(torch.isnan(got['d_gamma']).all()) and bool(torch.isfinite(got['d_beta']).all())


def test_add_ln_refusals():
    hip = pkg('hipops')
    lib, p, st = hip.lib(), hip._p, hip._stream()
    big = torch.zeros(8 * 1280 + 8, device=DEV)
    sd = torch.zeros(1, dtype=torch.int64, device=DEV)

    def fwd(a_ptr, adt, p_drop, c):
        return lib.ver_add_ln_forward(a_ptr, adt, p(big), p(big), p(big), p(sd), p_drop, H.EPS, p(big), None, p(big), p(big),
                                      2, c, st)

    def bwd(a_ptr, adt, p_drop, c):
        return lib.ver_add_ln_backward(p(big), None, a_ptr, adt, p(big), p(big), p(big), p(big), p(sd), p_drop, p(big), p(big),
                                       p(big), p(big), 2, c, st)

    for call in (fwd, bwd):
        for c in (128, 1280):
            _refused(lib, call(p(big), 0, 0.1, c), 'built for rows of 256, 512, 768 or 1024 channels (got %d)' % c)
        _refused(lib, call(p(big), 0, 1.0, 256), 'dropout probability 1 outside [0, 1)')
        for adt in (0, 1):
            _refused(lib, call(p(big) + 8, adt, 0.1, 256), 'buffers must be 16-byte aligned')
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ relu_dropout
def _relu_dropout(hip, r, n, dtype):
    lib, p, st = hip.lib(), hip._p, hip._stream()
    x, gy = r['inp']['x'].to(DEV), r['inp']['gy'].to(DEV)
    sd = torch.tensor([r['seed']], dtype=torch.int64, device=DEV) if r['p_drop'] > 0 else None   # (p = 0: may be NULL)
    guard = 64
    y, dx = _nan(n + guard, dtype), _nan(n + guard, dtype)
    _call(lib, lib.ver_relu_dropout_forward, p(x), p(y), p(sd), r['p_drop'], n, _code(dtype), st)
    _call(lib, lib.ver_relu_dropout_backward, p(y), p(gy), p(dx), r['p_drop'], n, _code(dtype), st)
    torch.cuda.synchronize()
    assert _untouched(y, n) and _untouched(dx, n)
    y, dx = y[:n], dx[:n]
    assert not bool(torch.isnan(y.float()).any()) and not bool(torch.isnan(dx.float()).any())     # written in full
    return dict(y=y, d_x=dx)


def _relu_dropout_case(n, dtype, p_drop, seed, device='cpu'):
    hip = pkg('hipops')
    r = H.relu_dropout_reference(n, dtype, p_drop, seed, device)
    got = {k: v.to(device) for k, v in _relu_dropout(hip, r, n, dtype).items()}
    keep, den, x = r['keep'], r['denormal'], r['inp']['x']
    for k in ('y', 'd_x'):
        assert bool((got[k][~keep] == 0).all()), k         # dropped by the host rule: exactly 0
    # the backward's only source of the gate is y -- denormal, infinite and overflowed values included
    assert torch.equal(got['d_x'] != 0, got['y'] != 0)
    model = r['models'][1]
    if p_drop == 0.0:                                      # bit-exact
        ity = torch.int32 if dtype == F32 else torch.int16
        assert torch.equal(got['y'][~den].view(ity), model['y'][~den].view(ity))
        assert torch.equal(got['d_x'][~den].view(ity), model['d_x'][~den].view(ity))
    if dtype == BF16:                                      # one rounding of the fp32 product
        for k in ('y', 'd_x'):
            assert bool(H.one_rounding(got[k], model[k + '32'])[~den].all()), k
    # a denormal x: never asserted against the model's gate (include/ver_ops.h): 0, or the model's value where it passed
    yd, md = got['y'][den].double(), r['exact']['y'][den].double()
    assert bool(((yd == 0) | ((yd - md).abs() <= md.abs() * 2.0 ** -6 + 2.0 ** -149)).all())
    if int(den.sum()):
        print('denormal x: %s -> y %s' % (x[den].double().tolist()[:4], yd.tolist()[:4]))
    _check('relu_dropout n=%d %s p=%g seed=%d' % (n, str(dtype)[6:], p_drop, seed), r, got)


@pytest.mark.parametrize('p_drop', [0.0, 0.1, 0.5])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', [4, 1020, 1028])
def test_relu_dropout_sizes_probabilities_seeds(n, dtype, p_drop):
    """one thread, a ragged workgroup, one thread into the second; +-0, the smallest normal, denormals, +inf and the largest
    finite value (times 1 / (1 - p): inf in model and kernel alike) written into x from 1 020 elements on; every seed."""
    for seed in H.SEEDS:
        _relu_dropout_case(n, dtype, p_drop, seed)


@pytest.mark.parametrize('p_drop,seed', [(0.1, 2 ** 62 - 1), (0.5, -1)])
@pytest.mark.parametrize('dtype', DTYPES)
def test_relu_dropout_second_trip(dtype, p_drop, seed):
    """16 384 x 256 x 4 + 1 028 elements: the second trip of the grid-stride loop with a ragged tail.  The mask is the host
    rule on every index; the fp64 chain and the models run on the device."""
    _relu_dropout_case(RELU_DROPOUT_TWO_TRIPS, dtype, p_drop, seed, DEV)


def test_relu_dropout_refusal():
    hip = pkg('hipops')
    lib, p, st = hip.lib(), hip._p, hip._stream()
    buf = torch.zeros(16, device=DEV)
    sd = torch.zeros(1, dtype=torch.int64, device=DEV)
    for n in (1, 6, 1021):
        _refused(lib, lib.ver_relu_dropout_forward(p(buf), p(buf), p(sd), 0.1, n, 0, st), 'element count must be a multiple of 4')
        _refused(lib, lib.ver_relu_dropout_backward(p(buf), p(buf), p(buf), 0.1, n, 0, st), 'element count must be a multiple of 4')


# ----------------------------------------------------------------------------------------------------------- ln_relu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', [1, 15, 16, 17, LN_RELU_TWO_TRIPS])
def test_ln_relu_on_gate_stable_rows(n, dtype):
    """around the 16 rows of a workgroup and into the second trip of the grid-stride loop (4 096 workgroups), ragged; from 15
    rows on with two rows of mean 100 (the last row among them) and a constant row, whose gates are the signs of beta."""
    hip = pkg('hipops')
    lib, p, st = hip.lib(), hip._p, hip._stream()
    r = H.ln_relu_reference(n, dtype)
    x, gy, g, b = (r[k].to(DEV).contiguous() for k in ('x', 'gy', 'gamma', 'beta'))
    rows = (n + 1) * 128
    y, mean, rstd, dx = _nan(rows, dtype), _nan(n + 1), _nan(n + 1), _nan(rows, dtype)
    dg, db = torch.full((128,), GARBAGE, device=DEV), torch.full((128,), -GARBAGE, device=DEV)
    _call(lib, lib.ver_ln_relu_forward, p(x), p(g), p(b), p(y), p(mean), p(rstd), n, 128, H.EPS, _code(dtype), st)
    _call(lib, lib.ver_ln_relu_backward, p(x), p(gy), p(g), p(b), p(mean), p(rstd), p(dx), p(dg), p(db), n, 128, _code(dtype), st)
    torch.cuda.synchronize()
    for name, buf, used in (('y', y, n * 128), ('mean', mean, n), ('rstd', rstd, n), ('d_x', dx, n * 128)):
        assert _untouched(buf, used), 'guard band of %s' % name
        assert bool(torch.isfinite(buf[:used].float()).all()), '%s was not written in full' % name
    got = dict(y=y[:n * 128].view(n, 128).cpu(), mean=mean[:n].cpu(), rstd=rstd[:n].cpu(), d_x=dx[:n * 128].view(n, 128).cpu(),
               d_gamma=dg.cpu(), d_beta=db.cpu())
    assert torch.equal(got['y'] != 0, r['gates'])
    if n >= 15:
        assert torch.equal(got['y'][7].float(), torch.relu(r['beta']).to(dtype).float())
    _check('ln_relu n=%d %s' % (n, str(dtype)[6:]), r, got)


def test_ln_relu_no_rows_and_refusals():
    hip = pkg('hipops')
    lib, p, st = hip.lib(), hip._p, hip._stream()
    dg, db = torch.full((128,), GARBAGE, device=DEV), torch.full((128,), -GARBAGE, device=DEV)
    _call(lib, lib.ver_ln_relu_backward, None, None, None, None, None, None, None, p(dg), p(db), 0, 128, 0, st)
    torch.cuda.synchronize()
    assert bool((dg == 0).all()) and bool((db == 0).all())
    buf = torch.zeros(4 * 256, device=DEV)
    for w in (64, 127, 256):
        _refused(lib, lib.ver_ln_relu_forward(p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), 2, w, H.EPS, 0, st),
                 'width %d (built for 128)' % w)
        _refused(lib, lib.ver_ln_relu_backward(p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), 2, w, 0,
                                                st), 'width %d (built for 128)' % w)
