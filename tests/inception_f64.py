"""Independent fp64 restatement of torchvision's InceptionV3 up to pool3 (the reference's FID network,
gan_training/metrics/inception.py) written from the layer table with F.conv2d -> F.batch_norm -> relu, BatchNorm NOT folded,
and synthetic weights that behave like trained ones.

synthetic_state_dict(seed): conv weights seeded normal (1 / sqrt(fan_in)), BN gamma ~ U(0.5, 1.5), beta ~ U(-0.2, 0.2), and
every BN's running mean / variance CALIBRATED: set unit by unit, in network order, to the batch statistics of that conv's
output on a fixed seeded calibration batch — activations then stay O(1) through all 94 units."""
import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _bc(name, ci, co, k=1, s=1, p=0):
    k = (k, k) if isinstance(k, int) else k
    s = (s, s) if isinstance(s, int) else s
    p = (p, p) if isinstance(p, int) else p
    return dict(name=name, ci=ci, co=co, k=k, s=s, p=p)


def _block_a(n, cin, pool):
    return [_bc(f'{n}.branch1x1', cin, 64), _bc(f'{n}.branch5x5_1', cin, 48), _bc(f'{n}.branch5x5_2', 48, 64, 5, p=2),
            _bc(f'{n}.branch3x3dbl_1', cin, 64), _bc(f'{n}.branch3x3dbl_2', 64, 96, 3, p=1),
            _bc(f'{n}.branch3x3dbl_3', 96, 96, 3, p=1), _bc(f'{n}.branch_pool', cin, pool)]


def _block_c(n, c7):
    return [_bc(f'{n}.branch1x1', 768, 192), _bc(f'{n}.branch7x7_1', 768, c7), _bc(f'{n}.branch7x7_2', c7, c7, (1, 7), p=(0, 3)),
            _bc(f'{n}.branch7x7_3', c7, 192, (7, 1), p=(3, 0)), _bc(f'{n}.branch7x7dbl_1', 768, c7),
            _bc(f'{n}.branch7x7dbl_2', c7, c7, (7, 1), p=(3, 0)), _bc(f'{n}.branch7x7dbl_3', c7, c7, (1, 7), p=(0, 3)),
            _bc(f'{n}.branch7x7dbl_4', c7, c7, (7, 1), p=(3, 0)), _bc(f'{n}.branch7x7dbl_5', c7, 192, (1, 7), p=(0, 3)),
            _bc(f'{n}.branch_pool', 768, 192)]


def _block_e(n, cin):
    return [_bc(f'{n}.branch1x1', cin, 320), _bc(f'{n}.branch3x3_1', cin, 384), _bc(f'{n}.branch3x3_2a', 384, 384, (1, 3), p=(0, 1)),
            _bc(f'{n}.branch3x3_2b', 384, 384, (3, 1), p=(1, 0)), _bc(f'{n}.branch3x3dbl_1', cin, 448),
            _bc(f'{n}.branch3x3dbl_2', 448, 384, 3, p=1), _bc(f'{n}.branch3x3dbl_3a', 384, 384, (1, 3), p=(0, 1)),
            _bc(f'{n}.branch3x3dbl_3b', 384, 384, (3, 1), p=(1, 0)), _bc(f'{n}.branch_pool', cin, 192)]


TABLE = ([_bc('Conv2d_1a_3x3', 3, 32, 3, 2), _bc('Conv2d_2a_3x3', 32, 32, 3), _bc('Conv2d_2b_3x3', 32, 64, 3, p=1),
          _bc('Conv2d_3b_1x1', 64, 80), _bc('Conv2d_4a_3x3', 80, 192, 3)]
         + _block_a('Mixed_5b', 192, 32) + _block_a('Mixed_5c', 256, 64) + _block_a('Mixed_5d', 288, 64)
         + [_bc('Mixed_6a.branch3x3', 288, 384, 3, 2), _bc('Mixed_6a.branch3x3dbl_1', 288, 64),
            _bc('Mixed_6a.branch3x3dbl_2', 64, 96, 3, p=1), _bc('Mixed_6a.branch3x3dbl_3', 96, 96, 3, 2)]
         + _block_c('Mixed_6b', 128) + _block_c('Mixed_6c', 160) + _block_c('Mixed_6d', 160) + _block_c('Mixed_6e', 192)
         + [_bc('Mixed_7a.branch3x3_1', 768, 192), _bc('Mixed_7a.branch3x3_2', 192, 320, 3, 2),
            _bc('Mixed_7a.branch7x7x3_1', 768, 192), _bc('Mixed_7a.branch7x7x3_2', 192, 192, (1, 7), p=(0, 3)),
            _bc('Mixed_7a.branch7x7x3_3', 192, 192, (7, 1), p=(3, 0)), _bc('Mixed_7a.branch7x7x3_4', 192, 192, 3, 2)]
         + _block_e('Mixed_7b', 1280) + _block_e('Mixed_7c', 2048))
UNIT = {u['name']: u for u in TABLE}
SUFFIXES = ('conv.weight', 'bn.weight', 'bn.bias', 'bn.running_mean', 'bn.running_var')


def table_keys():
    return {f"{u['name']}.{s}" for u in TABLE for s in SUFFIXES}


def forward_f64(sd, images, dims=2048, calibrate=False):
    """The reference wrapper's forward (inception.py:83-106) + fid_score.py:83-84's average pool, in fp64.
    calibrate=True: before each BN, its running statistics in `sd` are replaced by the conv output's batch statistics."""
    def bc(name, x):
        u = UNIT[name]
        w = sd[f'{name}.conv.weight'].double()
        y = F.conv2d(x, w, None, u['s'], u['p'])
        if calibrate:
            sd[f'{name}.bn.running_mean'] = y.mean((0, 2, 3)).float()
            sd[f'{name}.bn.running_var'] = y.var((0, 2, 3), unbiased=False).float()
        y = F.batch_norm(y, sd[f'{name}.bn.running_mean'].double(), sd[f'{name}.bn.running_var'].double(),
                         sd[f'{name}.bn.weight'].double(), sd[f'{name}.bn.bias'].double(), False, 0.0, 1e-3)
        return F.relu(y)

    def avg(x):
        return F.avg_pool2d(x, 3, 1, 1, count_include_pad=True)

    x = F.interpolate(images.double(), size=(299, 299), mode='bilinear', align_corners=False)
    x = x.clone()
    for c in range(3):
        x[:, c] = x[:, c] * (STD[c] / 0.5) + (MEAN[c] - 0.5) / 0.5
    for n in ('Conv2d_1a_3x3', 'Conv2d_2a_3x3', 'Conv2d_2b_3x3'):
        x = bc(n, x)
    x = F.max_pool2d(x, 3, 2)
    if dims == 64:
        return x.mean((2, 3))
    x = F.max_pool2d(bc('Conv2d_4a_3x3', bc('Conv2d_3b_1x1', x)), 3, 2)
    if dims == 192:
        return x.mean((2, 3))
    for m in ('Mixed_5b', 'Mixed_5c', 'Mixed_5d'):
        x = torch.cat([bc(f'{m}.branch1x1', x), bc(f'{m}.branch5x5_2', bc(f'{m}.branch5x5_1', x)),
                       bc(f'{m}.branch3x3dbl_3', bc(f'{m}.branch3x3dbl_2', bc(f'{m}.branch3x3dbl_1', x))),
                       bc(f'{m}.branch_pool', avg(x))], 1)
    m = 'Mixed_6a'
    x = torch.cat([bc(f'{m}.branch3x3', x), bc(f'{m}.branch3x3dbl_3', bc(f'{m}.branch3x3dbl_2', bc(f'{m}.branch3x3dbl_1', x))),
                   F.max_pool2d(x, 3, 2)], 1)
    for m in ('Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e'):
        b1 = bc(f'{m}.branch1x1', x)
        b7 = bc(f'{m}.branch7x7_3', bc(f'{m}.branch7x7_2', bc(f'{m}.branch7x7_1', x)))
        d = x
        for i in range(1, 6):
            d = bc(f'{m}.branch7x7dbl_{i}', d)
        x = torch.cat([b1, b7, d, bc(f'{m}.branch_pool', avg(x))], 1)
    if dims == 768:
        return x.mean((2, 3))
    m = 'Mixed_7a'
    b3 = bc(f'{m}.branch3x3_2', bc(f'{m}.branch3x3_1', x))
    b7 = x
    for i in range(1, 5):
        b7 = bc(f'{m}.branch7x7x3_{i}', b7)
    x = torch.cat([b3, b7, F.max_pool2d(x, 3, 2)], 1)
    for m in ('Mixed_7b', 'Mixed_7c'):
        b1 = bc(f'{m}.branch1x1', x)
        t = bc(f'{m}.branch3x3_1', x)
        b3 = torch.cat([bc(f'{m}.branch3x3_2a', t), bc(f'{m}.branch3x3_2b', t)], 1)
        t = bc(f'{m}.branch3x3dbl_2', bc(f'{m}.branch3x3dbl_1', x))
        bd = torch.cat([bc(f'{m}.branch3x3dbl_3a', t), bc(f'{m}.branch3x3dbl_3b', t)], 1)
        x = torch.cat([b1, b3, bd, bc(f'{m}.branch_pool', avg(x))], 1)
    return x.mean((2, 3))


_CACHE = {}


def synthetic_state_dict(seed=0):
    """torchvision-layout state_dict (fp32, CPU, plus num_batches_tracked and an fc head that the loader must ignore)."""
    if seed in _CACHE:
        return dict(_CACHE[seed])
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for u in TABLE:
        n, ci, co, (kh, kw) = u['name'], u['ci'], u['co'], u['k']
        sd[f'{n}.conv.weight'] = torch.randn(co, ci, kh, kw, generator=g) / (ci * kh * kw) ** 0.5
        sd[f'{n}.bn.weight'] = torch.rand(co, generator=g) + 0.5
        sd[f'{n}.bn.bias'] = torch.rand(co, generator=g) * 0.4 - 0.2
        sd[f'{n}.bn.running_mean'] = torch.zeros(co)
        sd[f'{n}.bn.running_var'] = torch.ones(co)
        sd[f'{n}.bn.num_batches_tracked'] = torch.tensor(0)
    sd['fc.weight'] = torch.randn(1000, 2048, generator=g) * 0.01
    sd['fc.bias'] = torch.zeros(1000)
    calib = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1000 + seed)) * 2 - 1
    with torch.no_grad():
        forward_f64(sd, calib, 2048, calibrate=True)
    _CACHE[seed] = sd
    return dict(sd)


def wrapper_layout(sd):
    """The same weights under the reference wrapper's keys (blocks.<i>.<j>.…)."""
    names = ['Conv2d_1a_3x3', 'Conv2d_2a_3x3', 'Conv2d_2b_3x3'], ['Conv2d_3b_1x1', 'Conv2d_4a_3x3'], \
        ['Mixed_5b', 'Mixed_5c', 'Mixed_5d', 'Mixed_6a', 'Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e'], \
        ['Mixed_7a', 'Mixed_7b', 'Mixed_7c']
    to = {m: f'blocks.{i}.{j}' for i, ms in enumerate(names) for j, m in enumerate(ms)}
    out = {}
    for k, v in sd.items():
        mod, rest = k.split('.', 1)
        if mod in to:
            out[f'{to[mod]}.{rest}'] = v
    return out
