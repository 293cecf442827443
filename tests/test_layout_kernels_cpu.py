"""layout_kernels_helper without a GPU: the models agree with independent statements of the same operations
(_cpu_algebra.from_plain, torch permutes and slices, the production plan's own index tables), every case is legal under the
launchers' rules, every case list reaches the launch forms it is named after, and each addressing fault a kernel of this
kind can have -- planted into a model -- changes the model's output on at least one case of the table that is meant to catch
it (test_layout_kernels_gpu.py holds the kernels to the same models, bit for bit)."""
import pytest
import torch

import layout_kernels_helper as K
from util import pkg

F32, BF16 = torch.float32, torch.bfloat16


def _plain(case, Z=None, kind='raw', seed=3):
    make = K.raw_data if kind == 'raw' else K.int_data
    return make((case['B'], Z or case.get('Zs') or case['Z'], case['H'], case['W'], case['C']), case['dtype'] if 'dtype' in case else BF16, seed)


# ------------------------------------------------------------------------------------------------------------ models
@pytest.mark.parametrize('layout', [0, 1, 2, 3])
def test_layouts_equal_the_cpu_algebra(layout):
    alg = pkg('dense_heads._cpu_algebra')
    plain = K.raw_data((2, 4, 4, 6, 8), BF16, 11)
    e = K.to_layout(plain, layout)
    assert K.same_bits(e, alg.from_plain(plain, layout))
    assert tuple(e.shape) == K.layout_shape(2, 4, 4, 6, 8, layout)
    assert K.same_bits(K.from_layout(e, layout, 2, 4, 4, 6), plain)
    assert K.same_bits(alg.to_plain(e, layout).contiguous(), plain)
    if layout < 2:                                                           # Z = 3: plain and planar only
        p3 = K.raw_data((2, 3, 4, 6, 4), F32, 12)
        assert K.same_bits(K.to_layout(p3, layout), alg.from_plain(p3, layout))


def test_tap_matrix_equals_padded_slices_and_its_adjoint_equals_autograd():
    """the same matrix from zero-padded slices (the way _cpu_algebra.im2col states it), Zr != Zs included; the adjoint from
    torch's autograd through those slices, in fp64"""
    F = torch.nn.functional
    for (Zs, Zr, taps) in ((4, 2, K.TAP_LISTS['max64']), (3, 3, K.TAP_LISTS['lat18']), (4, 2, K.TAP_LISTS['seven'])):
        B, H, W, C = 2, 4, 6, 8
        plain = K.int_data((B, Zs, H, W, C), F32, 5).double().requires_grad_(True)
        offs, _, stride = K.col_plan(len(taps), C, 1)
        pad = F.pad(plain, (0, 0, 8, 8, 8, 8, 4, 4))
        col = torch.full((B, Zr, H, W, stride), K.SENTINEL, dtype=torch.float64)
        parts = []
        for (dz, dy, dx), o in zip(taps, offs):
            parts.append((o, pad[:, 4 + dz:4 + dz + Zr, 8 + dy:8 + dy + H, 8 + dx:8 + dx + W]))
        for o, p in parts:
            col[..., o:o + C] = p.detach()
        got = K.gather_ref(plain.detach(), taps, offs, stride, Zr)
        assert torch.equal(got, col.view(-1, stride))
        g = K.int_data((B * Zr * H * W, stride), F32, 6).double()
        sum((p * g.view(B, Zr, H, W, stride)[..., o:o + C]).sum() for o, p in parts).backward()
        assert torch.equal(K.scatter_ref(g, taps, offs, B, Zr, Zs, H, W, C), plain.grad)
        assert K.max_terms(taps, B, Zr, Zs, H, W) <= len(taps)


def test_constant_blocks_repeat_per_sample_and_gaps_keep_the_sentinel():
    case = K.CONST_CASES[1]
    taps, offs, coffs, stride = K.case_geometry(case)
    plain = _plain(case)
    rps = case['Zr'] * case['H'] * case['W']
    const = K.raw_data((rps, case['nconst'], case['cw']), BF16, 9)
    col = K.gather_ref(plain, taps, offs, stride, case['Zr'], const=const, const_offs=coffs)
    assert K.same_bits(col[:rps, coffs[3]:coffs[3] + 16], const[:, 3]) and K.same_bits(col[rps:, coffs[3]:coffs[3] + 16], const[:, 3])
    owned = torch.zeros(stride, dtype=torch.bool)
    for o in offs:
        owned[o:o + case['C']] = True
    for o in coffs:
        owned[o:o + case['cw']] = True
    assert int((~owned).sum()) >= 8 * (len(taps) + 8) and bool((col[:, ~owned] == K.SENTINEL).all())


def test_channel_first_rows_equal_a_permute():
    plain = K.raw_data((2, 3, 4, 6, 5), F32, 2)
    cf = K.channel_first_ref(plain, 5 * 72 + 3)
    assert K.same_bits(cf[:, :360].reshape(2, 5, 3, 4, 6), plain.permute(0, 4, 1, 2, 3).contiguous())
    assert bool((cf[:, 360:] == K.SENTINEL).all())
    assert K.same_bits(K.from_channel_first(cf, 3, 4, 6, 5), plain)


def test_row_map_model_reproduces_the_production_plan():
    """the vocc geometry: the model, applied to the plan's own row map, names for every lattice element the operand element
    that the plan's gather table (built by brute force from the two raw views) reads it into"""
    opl = pkg('dense_heads.occ_proj_lattice')
    C, Z, Hl, Wl, bs = 768, 4, 60, 60, 2
    plan = opl.get_plan(C, Z, 2 * Hl, 2 * Wl, torch.device('cpu'))
    rm, spans, total = opl._row_map_for(plan, bs)
    assert rm['period'] == 960 and len(rm['seg_off']) == 5
    rm['total'] = total
    assert K.row_map_refusal(rm, Z, Hl, Wl, C) is None
    L = C * Z * Hl * Wl
    flat = torch.arange(L)
    for b in range(bs):
        dest = K.row_map_dest(flat, b, rm)
        tiled, wraps = K.row_map_dest_tiled(flat, b, rm, K.tile_rows(Hl, Wl, 2, True) * Wl)
        assert torch.equal(dest, tiled) and wraps >= 1
        where = torch.full((total,), -1, dtype=torch.int64)
        where[dest] = flat
        for g, (b0, n) in zip(plan.groups, spans):
            got = where[b0:b0 + n].view(bs, g.n_rows, g.k_aug)[b, :, :g.n_cols]
            assert torch.equal(got, g.gather_aug.view(g.n_rows, g.k_aug)[:, :g.n_cols])
            other = where[b0:b0 + n].view(bs, g.n_rows, g.k_aug)
            assert bool((other[:, :, g.n_cols:] == -1).all()) and bool((other[1 - b] == -1).all())


def test_run_copy_models_equal_index_select():
    for name in K.RUN_CASES[:-1]:
        c = K.run_case(name, BF16)
        image = K.raw_data((c['B'], c['image_stride']), BF16, 4)
        rows = K.run_gather_ref(image, c)
        idx = torch.cat([(c['run_start'].long()[:, :, None] + torch.arange(c['run_len'])).reshape(c['n_rows'], -1),
                         c['aug_idx'].long()], 1)
        want = image.index_select(1, idx.reshape(-1)).view(c['B'] * c['n_rows'], -1)
        ncol = want.shape[1]
        assert K.same_bits(rows[:, :ncol], want) and bool((rows[:, ncol:] == K.SENTINEL).all())
        if c['tiling']:
            full = K.raw_data((c['B'] * c['n_rows'], c['row_elems']), BF16, 5)
            img = K.run_scatter_ref(full, c)
            nrun = c['runs'] * c['run_len']
            assert K.same_bits(K.run_gather_ref(img, c)[:, :nrun], full[:, :nrun])
            assert bool((img[:, c['image_len']:] == K.SENTINEL).all())
            cover = torch.zeros(c['image_len'], dtype=torch.int64)
            cover.index_add_(0, idx[:, :nrun].reshape(-1), torch.ones(idx[:, :nrun].numel(), dtype=torch.int64))
            assert bool((cover == 1).all())                                    # the scatter runs tile the image exactly once
        else:
            assert len(set(idx[:, :c['runs'] * c['run_len']].reshape(-1).tolist())) < c['n_rows'] * c['runs'] * c['run_len']


def test_weight_models_equal_torch():
    for ci, co in K.PAIR_CASES + K.BLOCK_CASES:
        w = torch.randn(ci, co, 3, 5, 5, generator=torch.Generator().manual_seed(ci))
        k = K.taps_ref(w, F32)
        for a in range(3):
            for b in range(5):
                assert torch.equal(k[(a * 5 + b) * 5 + 1], w[:, :, 2 - a, 4 - b, 3])
        g = torch.randn(75, ci, co, generator=torch.Generator().manual_seed(co))
        w2 = w.clone().requires_grad_(True)
        (K.taps_ref(w2, F32) * g).sum().backward()
        assert torch.equal(K.taps_adjoint_ref(g), w2.grad)
    ci, co, ld = 5, 6, 16
    off, rows = K.block_offsets_case(ci, co, ld)
    w = K.int_data((ci, co, 3, 5, 5), F32, 1)
    blocks = K.forward_blocks_ref(w, off, ld, torch.full((rows, ld), K.SENTINEL))
    k = K.taps_ref(w, F32)
    t = 6                                               # lower half at slot 42, upper half at slot 69
    assert torch.equal(blocks[42 * ci:43 * ci, :co], k[t]) and torch.equal(blocks[69 * ci:70 * ci, co:2 * co], k[t])
    used = sum(int((off[:, h] >= 0).sum()) for h in range(2))
    assert int((blocks != K.SENTINEL).sum()) <= used * ci * co and int((blocks == K.SENTINEL).sum()) >= rows * ld - used * ci * co
    # the adjoint of the placement: <forward_blocks(w), s> == <w, backward_blocks(s)>
    s = K.int_data((rows, ld), F32, 2)
    placed = K.forward_blocks_ref(w, off, ld, torch.zeros(rows, ld))
    assert float((placed.double() * s.double()).sum()) == float((w.double() * K.backward_blocks_ref(s, off, ld, ci, co)).sum())
    sm, br, x, gv = K.vec_case(9, 520, F32)
    vec = K.blocks_vec_ref(sm[:, :520], br, 9, x)
    assert torch.equal(vec, torch.stack([x.double() @ sm[int(r):int(r) + 9, :520].double() for r in br]))
    gx = K.blocks_vec_adjoint_ref(sm[:, :520], br, 9, gv)
    assert float((vec * gv.double()).sum()) == float((gx * x.double()).sum())


# ------------------------------------------------------------------------------------------- legality and reach
def test_gather_scatter_cases_are_legal_and_reach_their_forms():
    names = [c['name'] for c in K.GATHER_CASES + K.CONST_CASES + K.STRIDE_GATHER + K.STRIDE_SCATTER]
    assert len(set(names)) == len(names)
    cvs = set()
    for c in K.GATHER_CASES + K.CONST_CASES + K.STRIDE_GATHER + K.STRIDE_SCATTER:
        taps, offs, coffs, stride = K.case_geometry(c)
        es = K.esize(c['dtype'])
        assert 1 <= len(taps) <= 64 and all(-127 <= v <= 127 for t in taps for v in t)
        assert K.layout_legal(c['layout'], c['Zs'], c['H'], c['W']) and (c['C'] * es) % 16 == 0 and (stride * es) % 16 == 0
        assert all(o >= 0 and o + c['C'] <= stride and (o * es) % 16 == 0 for o in offs)
        assert 0 <= c['nconst'] <= 8 and (c['cw'] * es) % 16 == 0
        assert all((o * es) % 16 == 0 and o + c['cw'] <= stride for o in coffs)
        spans = sorted([(o, o + c['C']) for o in offs] + [(o, o + c['cw']) for o in coffs])
        assert all(a[1] < b[0] for a, b in zip(spans, spans[1:]))                 # disjoint, with gaps
        assert sorted(offs) != offs or len(offs) == 1                              # permuted
        cvs.add(K.gather_form(1, c['C'], c['dtype'], len(taps))['CV'])
        if not K.scatter_form(1, c['C'], c['dtype'])['refuse']:
            K.exact_ok(K.max_terms(taps, 1, c['Zr'], c['Zs'], c['H'], c['W']))
    assert cvs >= {1, 3, 12, 96, 192, 320}
    form = {cv: K.gather_form(96, C, dt, 18) for dt, C, cv in K.CV_SWEEP}
    assert (form[12]['dt'], form[12]['dv']) == (21, 4) and (form[192]['dt'], form[192]['dv']) == (1, 64)
    assert all(form[cv]['dv'] == 0 for cv in (1,)) and form[3]['dv'] == 1 and form[96]['dv'] == 64
    assert K.gather_form(96, 1280, F32, 18)['dt'] == 0
    assert form[12]['trips'] == 1 and K.gather_form(96, 96, BF16, 64)['trips'] == 3 and form[96]['trips'] == 7 and form[192]['trips'] == 14
    assert any(c['C'] == 96 and c['taps'] == 'max64' for c in K.GATHER_CASES)        # CV = 12 beyond one trip
    sf = {cv: K.scatter_form(192, C, dt) for dt, C, cv in K.CV_SWEEP}
    assert sf[96]['G'] == 2 and sf[192]['G'] == 1 and sf[1]['G'] == 4 and sf[3]['idle'] == 244 and sf[12]['idle'] == 208
    assert sf[96]['idle'] == 64 and sf[192]['idle'] == 64 and K.scatter_form(192, 1280, F32)['refuse']
    import test_lattice_gemm_gpu
    assert K.LAT_TAPS == test_lattice_gemm_gpu.LAT_TAPS and len(K.LAT_TAPS) == 18
    m64 = K.TAP_LISTS['max64']
    assert len(m64) == 64 and len(set(m64)) == 64 and len(K.TAP_LISTS['seven']) % 6 == 1
    dead = [t for t in m64 if abs(t[1]) >= 4 or abs(t[2]) >= 6 or t[0] >= 4]
    assert len(dead) >= 4 and all(len(r) == 0 for (r, _), t in zip(K.selection(m64, 1, 2, 4, 4, 6), m64) if t in dead)
    assert K.max_terms(m64, 1, 2, 4, 4, 6) > 6                                     # more than one six-wide batch of live taps
    wide = K.CONST_CASES[2]
    assert wide['nconst'] * (wide['cw'] * 2 // 16) > 256
    for c, want in zip(K.STRIDE_GATHER, (8640, 16815)):
        f = K.gather_form(c['B'] * c['Zr'] * c['H'] * c['W'], c['C'], c['dtype'], 2)
        assert c['B'] * c['Zr'] * c['H'] * c['W'] == want and f['strided']
    assert K.gather_form(16815, 8, BF16, 2)['rows_per_group'] == 3 and 16815 % 2 == 1
    c = K.STRIDE_SCATTER[0]
    sf = K.scatter_form(c['B'] * c['Zs'] * c['H'] * c['W'], c['C'], c['dtype'])
    assert c['B'] * c['Zs'] * c['H'] * c['W'] == 33600 > 32768 and sf['strided'] and sf['G'] == 4


def test_gather_walk_names_every_vector_once():
    for cv, ntaps in ((1, 18), (3, 7), (12, 18), (96, 64), (192, 18), (320, 18), (320, 64), (3, 64)):
        assert sorted(K.gather_walk(cv, ntaps)) == [(t, v) for t in range(ntaps) for v in range(cv)], (cv, ntaps)


def test_im2col_cases_reach_the_grid_cap():
    assert not K.im2col_form(2 * 4 * 40 * 40, 80, 8, BF16)['strided']              # 1 024 000 vectors: under the cap of 2 097 152
    assert K.im2col_form(2 * 4 * 60 * 56, 80, 8, BF16)['strided']                  # 2 150 400
    assert len(K.TAPS80) == 80 == len(set(K.TAPS80))
    for name, (B, Z, H, W, C, dtype, taps) in K.IM2COL_CASES.items():
        f = K.im2col_form(B * Z * H * W, len(taps), C, dtype)
        assert f['strided'] == (name == 'grid_cap') and (C * K.esize(dtype)) % 16 == 0
        K.exact_ok(K.max_terms(taps, 1, Z, Z, H, W))
    assert K.max_terms(K.TAPS80, 1, 4, 4, 5, 7) > 27


def test_transpose_cases_reach_their_forms():
    for c in K.TRANSPOSE_CASES:
        L = c['C'] * c['Z'] * c['H'] * c['W']
        assert K.transpose_layouts(c), c['name']
        for to_cf in (True, False):
            f = K.transpose_form(c['B'], c['Z'], c['H'], c['W'], c['C'], c['dtype'], to_cf, L + c['tail'], c['cf_offset'])
            assert f['form'] == c['want'], (c['name'], f)
            if c['fails']:
                assert [k for k, ok in f['pre'].items() if not ok] == [c['fails']], (c['name'], f['pre'])
            if c['R'] and to_cf:
                assert f['R'] == c['R'] and f['hr'] > 1
            assert f['lds'] <= 64 * 1024
    tb = K.transpose_form(2, 4, 16, 64, 40, BF16, True, 40 * 4096 + 8)
    assert (tb['R'], tb['hr'], tb['blocks']) == (8, 2, 2)
    assert K.transpose_form(2, 4, 16, 64, 40, BF16, False, 40 * 4096 + 8)['blocks'] == 1
    tf = K.transpose_form(2, 4, 16, 32, 36, F32, True, 36 * 2048 + 8)
    assert (tf['R'], tf['hr'], tf['blocks']) == (8, 2, 2)
    assert K.transpose_form(2, 1, 2, 126, 4, F32, True, 1016)['lds'] == 65024
    assert K.transpose_form(2, 1, 2, 128, 4, F32, True, 1032)['form'] == 'refuse'
    assert K.transpose_form(0, 1, 2, 128, 4, F32, True, 1032)['form'] == 'none'
    assert all(K.transpose_layouts(c) == [0, 1, 2, 3] for c in K.TRANSPOSE_CASES[:4])
    # Z H W % vx != 0 cannot fail alone: W % vx == 0 implies it.  Z = 1 and Z = 3 run the vector form on layouts 0 and 1.
    for c in K.TRANSPOSE_CASES:
        vx = 8 // K.esize(c['dtype'])
        assert c['W'] % vx or (c['Z'] * c['H'] * c['W']) % vx == 0
    assert [K.transpose_layouts(c) for c in K.TRANSPOSE_CASES[4:6]] == [[0, 1], [0, 1]]


def test_rows_cases_are_legal_and_reach_their_forms():
    a = [c for c in K.ROWS_CASES if c['name'].startswith('A_')]
    assert len(a) >= 6
    print('legal geometry-A combinations:', [c['name'] for c in a])
    seen = dict(wraps=set(), nseg=set(), k0=False, plane=False, long=False)
    for c in K.ROWS_CASES:
        rm = c['rm']
        assert K.row_map_refusal(rm, c['Z'], c['H'], c['W'], c['C']) is None, c['name']
        L = c['C'] * c['Z'] * c['H'] * c['W']
        need = max(b + c['B'] * r * p for b, r, p in zip(rm['seg_base'], rm['seg_rows'], rm['seg_pitch']))
        assert need <= rm['total'] and rm['seg_base'] == sorted(rm['seg_base'], reverse=True)
        assert all(p > (L // rm['quarter']) * s for p, s in zip(rm['seg_pitch'], rm['seg_len']))      # slack
        f = K.rows_form(c['Z'], c['H'], c['W'], c['C'], rm, True)
        flat = torch.arange(L)
        for P in (f['run'], c['W']):                      # both directions' tile runs lead to the definition's element
            tiled, _ = K.row_map_dest_tiled(flat, 1, rm, P)
            assert torch.equal(tiled, K.row_map_dest(flat, 1, rm))
        dest = torch.cat([K.row_map_dest(flat, b, rm) for b in range(c['B'])])
        assert len(set(dest.tolist())) == c['B'] * L and int(dest.max()) < rm['total']
        if c['name'].startswith('A_'):
            assert f['run'] == 64 and f['hr'] == 1
            seen['wraps'].add(f['wraps'])
            seen['nseg'].add(f['nseg'])
            seen['k0'] |= f['k_max'] == 0
            seen['plane'] |= rm['quarter'] == 64
            seen['long'] |= rm['period'] > f['run']
    assert seen['wraps'] >= {0, 1, 3} and seen['nseg'] >= {1, 2, 8} and seen['k0'] and seen['plane'] and seen['long']
    assert {c['C'] for c in a} == {16, 40}
    b = next(c for c in K.ROWS_CASES if c['name'] == 'B_tiles')
    assert K.rows_form(4, 16, 64, 8, b['rm'], True)['hr'] == 2
    last = next(c for c in K.ROWS_CASES if c['name'] == 'C_last_slot')
    f = K.rows_form(4, 16, 16, 16, last['rm'], True)
    assert f['slots'] == 1024 and last['rm']['quarter'] == last['rm']['period'] == 4096
    # the refusals of the GPU test are refusals by the launcher's rules
    assert K.row_map_refusal(K.make_row_map(8 * 4 * 4100, 4100, 4100, (4100,), 1), 4, 205, 20, 8) == 'period > 4096 or a plane straddles two quarters'
    short = K.make_row_map(4096, 1024, 64, (4, 56), 2)
    assert K.row_map_refusal(short, 4, 8, 8, 16) == 'cover'
    assert K.row_map_refusal(K.make_row_map(16 * 4 * 8 * 6, 48, 16, (16,), 2), 4, 8, 6, 16) == 'W % 4, C % 8'


def test_run_copy_cases_reach_their_forms():
    for dtype in (F32, BF16):
        forms = {}
        for name in K.RUN_CASES:
            c = K.run_case(name, dtype)
            ve = 8 // K.esize(dtype)
            assert c['run_len'] % ve == 0 and c['image_stride'] % ve == 0 and c['row_elems'] % ve == 0
            assert bool((c['run_start'] % ve == 0).all()) and int(c['run_start'].max()) + c['run_len'] <= c['image_len']
            assert c['row_elems'] >= c['runs'] * c['run_len'] + c['n_aug']
            forms[name] = K.run_copy_form(c['B'] * c['n_rows'], c['runs'], c['run_len'], c['n_aug'], dtype, True)
        assert [forms[n]['tail'] for n in ('tail1', 'tail2', 'tail3')] == [1, 2, 3]
        assert all(forms[n]['form'] == 'rows' for n in ('tail1', 'tail2', 'tail3', 'overlap', 'stride'))
        assert forms['flat']['form'] == 'flat' and forms['flat']['per_row'] == 305
        assert K.run_copy_form(7, 3, K.run_case('flat', dtype)['run_len'], 0, dtype, False)['per_row'] == 300
        assert forms['stride']['strided'] and forms['stride']['grid'] == 16384 and forms['stride']['tail'] == 1
        big = [K.run_case(n, dtype) for n in ('tail2', 'tail3')]
        assert all(c['row_elems'] > c['runs'] * c['run_len'] + c['n_aug'] and c['image_stride'] > c['image_len'] for c in big)
        assert K.run_case('tail1', dtype)['n_aug'] == 0 and K.run_case('tail2', dtype)['n_aug'] == 3


def test_weight_cases_reach_their_forms():
    assert [ci * co for ci, co in K.PAIR_CASES] == [35, 129, 64]
    assert [ci * co % 64 for ci, co in K.PAIR_CASES] == [35, 1, 0]
    assert all(co % 2 == 0 for _, co in K.BLOCK_CASES) and [ci * co for ci, co in K.BLOCK_CASES] == [30, 132]
    for ci, co in K.BLOCK_CASES:                        # even pitch and offsets (4-byte / 8-byte accesses), disjoint blocks inside the matrix
        ld = 2 * co + 4
        off, rows = K.block_offsets_case(ci, co, ld)
        live = off[off >= 0]
        assert ld % 2 == 0 and bool((live % 2 == 0).all()) and len(set(live.tolist())) == len(live)
        assert int(live.max()) + (ci - 1) * ld + co <= rows * ld and bool((off[:, 0] < 0).any()) and bool((off[:, 1] >= 0).any())
        assert all(int(o) % ld + co <= ld and int(o) // ld % ci == 0 for o in live)
    f = K.blocks_vec_form(9, 520)
    assert f['xblocks'] == 2 and f['live_last'] == 4 and f['slices'] == [2, 2, 2, 2, 1, 0, 0, 0]
    assert K.blocks_vec_form(1, 520)['slices'] == [1, 0, 0, 0, 0, 0, 0, 0]
    _, br, _, _ = K.vec_case(9, 520, F32)
    assert len(set(br.tolist())) < len(br) and br.tolist() != sorted(br.tolist())
    for ci, ncols in K.VEC_CASES:
        assert ci * 16 < 2 ** 24 and len(K.vec_case(ci, ncols, F32)[1]) * ncols * 16 < 2 ** 24      # exact partial sums in fp32
    sp = K.weight_specials()
    assert bool(torch.isinf(sp).any()) and bool((sp.abs() < 1e-38).any())
    r = sp.to(BF16).view(torch.int16).tolist()
    assert r[0] == 0x3F80 and r[1] == 0x3F82 and r[2] == 0x3F80 and r[3] == 0x3F81                 # ties to even, both ways


# ---------------------------------------------------------------------------------------------------- fault seeding
def _differs(table, right, wrong):
    hit = [c['name'] if isinstance(c, dict) else str(c) for c in table if not K.same_bits(right(c), wrong(c))]
    return hit


def test_seeded_faults_change_the_models():
    """each wrong variant differs from the right model on at least one case of the table that is there to catch it"""
    small = [c for c in K.GATHER_CASES if c['C'] <= 96 or c['name'] in ('cv96_bf16_l0', 'cv192_f32_l3')]

    def gather(c, **kw):
        taps, offs, _, stride = K.case_geometry(c)
        return K.gather_ref(_plain(c), taps, offs, stride, c['Zr'], **kw)
    hit = _differs(small, gather, lambda c: gather(c, swap_xy=True))
    assert len(hit) == len(small), 'x / y swapped in the taps'

    def walked(c, wrap):
        taps, offs, _, stride = K.case_geometry(c)
        return K.gather_by_walk(gather(c), taps, offs, c['C'], c['dtype'], wrap)
    assert not _differs(small, gather, lambda c: walked(c, True))
    hit = _differs(small, gather, lambda c: walked(c, False))
    # (a row of at most 256 vectors is one trip: the walk never advances, whatever CV is)
    assert sorted(hit) == ['cv192_f32_l3', 'cv96_bf16_l0', 'max64_cv12_l1', 'max64_cv12_l2'], "the gather's v >= CV wrap dropped"

    def stored(c, **kw):
        return K.to_layout(_plain(c), c['layout'], **kw).reshape(-1)
    hit = _differs(small, stored, lambda c: stored(c, swap_parity=True))
    assert hit and {c['layout'] for c in small if c['name'] in hit} == {1, 3}, 'the plane parity bit swapped'

    def cf(c, **kw):
        return K.channel_first_ref(_plain(c), c['C'] * c['Z'] * c['H'] * c['W'] + c['tail'], **kw)
    hit = _differs(K.TRANSPOSE_CASES, cf, lambda c: cf(c, swap_xy=True))
    assert len(hit) == len(K.TRANSPOSE_CASES), 'x / y swapped in the channel-first rows'

    def y0(c):
        f = K.transpose_form(c['B'], c['Z'], c['H'], c['W'], c['C'], c['dtype'], True, c['C'] * c['Z'] * c['H'] * c['W'] + c['tail'], c['cf_offset'])
        return cf(c, y0_zero_R=f['R'] if f['form'] == 'vector' else None)       # (the scalar kernel has no spatial tiles)
    assert sorted(_differs(K.TRANSPOSE_CASES, cf, y0)) == ['tiles_bf16', 'tiles_f32'], 'y0 forced to 0'

    def rows(c, wrap=True):
        P = K.rows_form(c['Z'], c['H'], c['W'], c['C'], c['rm'], True)['run']
        return K.lattice_rows_ref(_plain(c), c['rm'], dest=lambda flat, b, rm: K.row_map_dest_tiled(flat, b, rm, P, wrap)[0] % rm['total'])
    some = [c for c in K.ROWS_CASES if c['C'] <= 16]
    assert not _differs(some, lambda c: K.lattice_rows_ref(_plain(c), c['rm']), rows)
    hit = _differs(some, rows, lambda c: rows(c, False))
    assert hit and all('p256' not in n or n.startswith('B_') for n in hit) and any('p16' in n for n in hit), 'a piece that does not wrap'

    def run(name, **kw):
        c = K.run_case(name, BF16)
        return K.run_gather_ref(K.raw_data((c['B'], c['image_stride']), BF16, 8), c, **kw)
    assert sorted(_differs(K.RUN_CASES[:3], run, lambda n: run(n, dup_tail=True))) == ['tail2', 'tail3'], 'the tail row duplicated'

    def run_back(name, **kw):
        c = K.run_case(name, BF16)
        return K.run_scatter_ref(K.raw_data((c['B'] * c['n_rows'], c['row_elems']), BF16, 8), c, **kw)
    assert sorted(_differs(K.RUN_CASES[:3], run_back, lambda n: run_back(n, dup_tail=True))) == ['tail2', 'tail3']

    def taps(p, **kw):
        return K.taps_ref(K.raw_data(p + (3, 5, 5), F32, 3), F32, **kw)
    assert len(_differs(K.PAIR_CASES, taps, lambda p: taps(p, flip=(2,)))) == 3, 'the tap flip on one axis only'
    assert _differs(K.PAIR_CASES, taps, lambda p: taps(p, skip_ragged=True)) == ['(5, 7)', '(3, 43)'], 'the ragged group skipped'
