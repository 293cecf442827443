"""Byte labels through the separate focal-loss passes, without a GPU: the four ``_u8`` entries are declared in the header,
bound by ``hipops`` and exported, their argument checks answer before any launch, and ``FocalLoss`` refuses uint8 targets
on the CPU as every wrapper of a HIP kernel refuses CPU tensors."""
import ctypes

import pytest
import torch

from util import pkg

U8_ENTRIES = ('ver_focal_loss_forward_u8', 'ver_focal_loss_backward_u8', 'ver_focal_loss_forward_u8_cw',
              'ver_focal_loss_backward_u8_cw')


def test_u8_entries_prototypes_and_argument_checks():
    hip = pkg('hipops')
    lib = hip.lib()
    assert set(U8_ENTRIES) <= set(hip.SYMBOLS) and set(U8_ENTRIES) <= set(hip.prototypes())
    # every byte entry has the argument list of its int64 twin (only the pointee of `target` differs)
    for name in U8_ENTRIES:
        assert hip.PROTOTYPES[name] == hip.PROTOTYPES[name.replace('_u8', '')], name
        assert getattr(lib, name).argtypes == hip.PROTOTYPES[name][1] and getattr(lib, name).restype is ctypes.c_int
    assert lib.ver_abi_version() == 31 == hip.ABI_VERSION       # additive: the version stays
    buf = torch.zeros(1024)                                     # host memory, 64-byte aligned; nothing is launched below
    p = buf.data_ptr()
    L, f = ctypes.c_long, ctypes.c_float

    def call(name, n, c, logits=p, out=p, table=p):
        fn = getattr(lib, name)
        common = (L(n), c, f(2.0), f(0.25), 0)
        if name == 'ver_focal_loss_forward_u8':
            return fn(logits, p, out, *common, None, None)
        if name == 'ver_focal_loss_backward_u8':
            return fn(logits, p, p, out, *common, None)
        if name == 'ver_focal_loss_forward_u8_cw':
            return fn(logits, p, table, out, *common, None, None)
        return fn(logits, p, table, p, out, *common, None)

    for name in U8_ENTRIES:
        assert call(name, 8, 10) == -2 and b'multiple of 8' in lib.ver_last_error(), name       # VER_EUNSUPPORTED
        assert call(name, -1, 16) == -1, name                                                   # VER_EINVAL
        assert call(name, 8, 16, logits=None) == -1 and b'null pointer' in lib.ver_last_error(), name
        assert call(name, 8, 16, logits=p + 4) == -1 and b'aligned' in lib.ver_last_error(), name
        assert call(name, 8, 16, out=None) == -1 and name.encode() in lib.ver_last_error(), name
    for name in U8_ENTRIES[:2]:                                 # byte labels: 254 classes and the empty label at most
        assert call(name, 8, 256) == -1 and b'byte labels' in lib.ver_last_error(), name
    for name in U8_ENTRIES[2:]:                                 # (the staged table is the narrower limit of the weighted forms)
        assert call(name, 8, 256) == -2 and b'class weights' in lib.ver_last_error(), name
        assert call(name, 8, 16, table=None) == -1 and b'class_weight' in lib.ver_last_error(), name
    for name in U8_ENTRIES[1:]:                                 # N == 0: nothing to launch
        assert call(name, 0, 16) == 0, name


@pytest.mark.parametrize('rows', [16, 5000])
def test_focal_loss_refuses_uint8_targets_on_the_cpu(rows):
    pkg()
    losses = pkg('dense_heads.losses')
    fl = losses.FocalLoss(use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0)
    gen = torch.Generator().manual_seed(rows)
    pred = torch.randn(rows, 16, generator=gen)
    target = torch.randint(0, 17, (rows,), generator=gen)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        fl(pred, target.to(torch.uint8), avg_factor=3.0)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        fl(pred, target.to(torch.uint8), avg_factor=3.0, class_weight=torch.ones(17))
    assert torch.isfinite(fl(pred, target, avg_factor=3.0))    # the int64 caller is untouched
    with pytest.raises(RuntimeError, match='GPU tensor'):      # ... and so is the wrapper's own refusal
        pkg('hipops').sigmoid_focal_loss_sum(pred, target.to(torch.uint8))
