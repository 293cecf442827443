"""What the tests of the flat gradient exchange share (tests/test_grad_exchange_gpu.py): the tensor sizes and gradient
values of the kernel tests, and the five-step scripts of the two captured training steps with their bounds.

The bounds of the five-step scripts are those of ``test_graphed_lift_step_replays_the_eager_training_steps``
(tests/test_head_gpu.py) and of tests/test_train_graph_gpu.py, the project's bound for "same kernels, replayed": losses within
1e-5 (fp32) / 2e-3 (bf16 autocast) relative, the update of every parameter within 0.05 / 0.2 relative L2.  AdamW's early
updates are ~ lr * sign(g): an element whose tiny gradient changes sign between two runs (the gather backward adds with fp32
atomics, so gradients differ in their last bits from run to run) moves by 2 lr, so the bound is on a tensor's update, not
element-wise.  The optimizer is ``ClipAdamW(lr=1e-6, eps=0.1)`` for the reason tests/test_train_graph_gpu.py's docstring
measures: with eps far above sqrt(v) an element's update is proportional to its gradient and rounding noise moves nothing,
so two EAGER runs stay inside these bounds, which they do not at eps = 1e-8.  An exchange adds to that: nothing on an fp32
wire (the flat step is bit for bit the pointer-table step), one bf16 rounding of every gradient on a bf16 wire -- which is why
the twin of the bf16 run is an eager EXCHANGED step: both sides round alike."""
import numpy as np
import torch

import cases
from util import pkg

T = torch.from_numpy
DEV = torch.device('cuda', 0)
# the chunk edges of ClipAdamW.CHUNK = 32768 and the vector tails (4 elements per lane of the step, 8 of the bf16 pack)
SIZES = (1, 3, 4, 7, 8, 9, 255, 256, 1023, 32767, 32768, 32769, 65541)
OFF4, OFF8 = 8, 9                      # indices in SIZES of the gradients that are views 4 / 8 bytes off a 16-byte boundary
LR, EPS = 1e-6, 0.1


def special_values():
    f32 = np.float32
    bits = np.array([1, 0x7fff, 0x8000, 0x8001, 0x007fffff, 0x00800000, 0x00018000], dtype=np.uint32).view(f32)
    v = np.concatenate([np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, np.finfo(f32).max, 0.0, np.inf, np.nan], dtype=f32), bits])
    return np.concatenate([v, -v])


def gradient_values(seed, specials=True):
    """One fp32 array per size: seeded normals * 0.01, the special values in the leading elements where they fit."""
    rng = np.random.default_rng(seed)
    sp = special_values()
    out = []
    for n in SIZES:
        g = (rng.standard_normal(n) * 0.01).astype(np.float32)
        if specials and n >= 255:
            g[:len(sp)] = sp
            g[-len(sp):] = sp[::-1]                # ... and in the tail elements, which the scalar loops take
        elif specials:
            g[:] = sp[(np.arange(n) + n) % len(sp)]
        out.append(g)
    return out


def gradient_tensors(values):
    """The values on the GPU as gradient tensors: 16-byte aligned, except the two views one and two elements into a larger
    buffer (a DistributedDataParallel bucket view looks like that)."""
    out = []
    for i, g in enumerate(values):
        lead = 1 if i == OFF4 else 2 if i == OFF8 else 0
        buf = torch.zeros(len(g) + 4, device=DEV)
        t = buf[lead:lead + len(g)]
        t.copy_(T(g))
        assert t.data_ptr() % 16 == 4 * lead
        out.append(t)
    return out


def bits(t):
    """A float tensor as integers on the host: bitwise comparison, NaNs included."""
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def same_losses(got, want, autocast, what):
    """Prints every figure, then returns the steps outside the bound."""
    tol = 2e-3 if autocast else 1e-5
    assert len(got) == len(want)
    outside = []
    for it, (g, w) in enumerate(zip(got, want)):
        ok = abs(g - w) <= tol * abs(w)
        print('%s step %d: %.9g vs %.9g%s' % (what, it, g, w, '' if ok else '   <-- outside %g' % tol))
        if not ok:
            outside.append((it, g, w))
    return outside


def same_updates(head, twin, before, autocast, what):
    """Prints the worst figure, then returns the parameters outside the bound as (name, relative difference)."""
    worst, outside = 0.0, []
    for (k, p), q in zip([(k, p) for k, p in twin.named_parameters() if p.requires_grad],
                         [q for q in head.parameters() if q.requires_grad]):
        d_e, d_g = (p.detach() - before[k]).double(), (q.detach() - before[k]).double()
        if float(d_e.norm()) == 0:
            if float(d_g.norm()) != 0:
                outside.append((k, float('inf')))
            continue
        r = float((d_e - d_g).norm() / d_e.norm())
        worst = max(worst, r)
        if not r < (0.2 if autocast else 0.05):
            outside.append((k, r))
    print('%s, %s: worst relative difference of a parameter update %.2e; outside the bound: %s'
          % (what, 'bf16' if autocast else 'fp32', worst, outside))
    return outside


class LiftModel(torch.nn.Module):
    """bench.py's LiftTrainer at one micro-batch: (feats, w2p, org, gt) -> occupancy loss (tests/test_head_gpu.py)."""

    def __init__(self, head, autocast):
        super().__init__()
        self.head, self.autocast = head, autocast

    def forward(self, feats, w2p, org, gt):
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=self.autocast):
            emb = self.head(feats, None, only_bev=True, world2pixel=w2p, origin=org)
            return self.head.occupancy_loss_from_volume(emb, gt)


LIFT = ('transformer.encoder.', 'transformer.level_embeds', 'transformer.cams_embeds', 'voxel_embedding.', 'up_sample.',
        'occ_proj.', 'occ_branches.')


def lift_head(seed=7):
    """The seeded vocc head of ``test_graphed_lift_step_replays_the_eager_training_steps`` with the lifting path trainable."""
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    pkg()
    h = pkg('registry').build_head(cases.vocc_head_cfg()).eval()
    code_weights = h.code_weights.detach().clone()
    pkg('synthetic').load_seeded(h, seed)
    h.code_weights.data.copy_(code_weights)
    h = h.to(DEV)
    for k, p in h.named_parameters():
        p.requires_grad_(k.startswith(LIFT))
    return h


def lift_inputs():
    syn = pkg('synthetic')
    w2p, org = syn.camera_batch(2, seed=1)
    feats = T(syn.vit_features(2, seed=0)).to(DEV)
    gts = T(np.random.default_rng(3).integers(0, 17, size=(2, 1, 504000))).to(DEV)
    return [(feats[b].unsqueeze(1).contiguous(), T(w2p[b:b + 1]).to(DEV), T(org[b:b + 1]).to(DEV), gts[b]) for b in range(2)]


def trainable(module):
    return [(k, p) for k, p in module.named_parameters() if p.requires_grad]


def optimizer(module, **kw):
    kw = dict(dict(lr=LR, eps=EPS, weight_decay=0.01, max_norm=35.0), **kw)
    return pkg('optim').ClipAdamW([p for _, p in trainable(module)], **kw)


def eager_steps(model, opt, exchange, batches, total=lambda out: out):
    """The steps of ``batches`` taken eagerly -- through the exchange when there is one -- -> what ``model`` returned, as
    floats (a loss, or a dict of them)."""
    outs = []
    for batch in batches:
        opt.zero_grad(set_to_none=True)
        out = model(*batch)
        total(out).backward()
        if exchange is None:
            opt.step()
        else:
            exchange.pack()
            exchange.all_reduce()
            opt.step(exchange=exchange)
        outs.append({k: float(v) for k, v in out.items()} if isinstance(out, dict) else float(out))
    out = None
    opt.zero_grad(set_to_none=True)
    return outs
