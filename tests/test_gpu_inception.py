"""GPU: the InceptionV3 feature extractor's HIP kernels (rick_amd/csrc/inception.hip) against fp64 torch, the whole network
against the independent fp64 restatement (tests/inception_f64.py), and the extractor inside the FID loop."""
import pytest
import torch
import torch.nn.functional as F

from tests.inception_f64 import forward_f64, synthetic_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = 12345.0


def _lib():
    from rick_amd import _lib
    return _lib


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _conv(x_nhwc, w, b, s, p, dsts, bn=None):
    """rick_inc_conv_f32 on w [Co, Ci, kh, kw] (Co = the concatenation of the segments), dsts = [(tensor, ldc, c0, ncols)]."""
    from rick_amd import gemm_conv
    N, IH, IW, Ci = x_nhwc.shape
    wpk, bp, Cop, bn = gemm_conv.pack(w, b, bn=bn)
    wpk, bp = wpk.to(DEV), bp.to(DEV)
    a = gemm_conv.descriptor(N, IH, IW, Ci, w.shape[2:], s, p, Cop, bn, [(t.data_ptr(), ldc, c0, nc) for t, ldc, c0, nc in dsts])
    gemm_conv.forward(x_nhwc.data_ptr(), wpk.data_ptr(), bp.data_ptr(), a)
    torch.cuda.synchronize()
    return a.OH, a.OW


def _rel(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize('hw', [(256, 256), (128, 128), (300, 280), (32, 48), (299, 299)])
def test_input_kernel_vs_fp64(hw):
    from rick_amd.inception import MEAN, STD
    L = _lib()
    x = torch.rand(3, 3, *hw, generator=torch.Generator().manual_seed(1)) * 2 - 1
    out = torch.full((3, 299, 299, 4), SENTINEL, device=DEV)
    L.check(L.lib.rick_inc_input_f32(x.to(DEV).data_ptr(), out.data_ptr(), 3, hw[0], hw[1], 299, 299, L.stream_ptr()),
            'rick_inc_input_f32')
    r = F.interpolate(x.double(), (299, 299), mode='bilinear', align_corners=False)
    ref = torch.stack([r[:, c] * (STD[c] / 0.5) + (MEAN[c] - 0.5) / 0.5 for c in range(3)], -1)
    got = out.cpu()
    assert torch.all(got[..., 3] == 0)
    # fp32 source coordinates (as torch's own fp32 kernel computes them): ~ulp(300) = 3e-5 of a pixel step
    assert float((got[..., :3].double() - ref).abs().max() / ref.abs().max()) < 1e-4


# every convolution geometry of the layer table: (Ci, Co, k, s, p)
GEOMS = [(4, 32, (3, 3), (2, 2), (0, 0)), (32, 32, (3, 3), (1, 1), (0, 0)), (32, 64, (3, 3), (1, 1), (1, 1)),
         (64, 80, (1, 1), (1, 1), (0, 0)), (80, 192, (3, 3), (1, 1), (0, 0)), (48, 64, (5, 5), (1, 1), (2, 2)),
         (96, 96, (3, 3), (2, 2), (0, 0)), (288, 384, (3, 3), (2, 2), (0, 0)), (128, 128, (1, 7), (1, 1), (0, 3)),
         (160, 192, (7, 1), (1, 1), (3, 0)), (384, 384, (1, 3), (1, 1), (0, 1)), (384, 384, (3, 1), (1, 1), (1, 0)),
         (448, 384, (3, 3), (1, 1), (1, 1)), (192, 320, (3, 3), (2, 2), (0, 0)), (2048, 192, (1, 1), (1, 1), (0, 0))]


@pytest.mark.parametrize('bn', [64, 128])
@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: f'{g[0]}-{g[1]}-k{g[2][0]}x{g[2][1]}-s{g[3][0]}-p{g[4][0]}{g[4][1]}')
def test_conv_geometry_into_channel_slice(geom, bn):
    ci, co, k, s, p = geom
    g = torch.Generator().manual_seed(ci * 7 + co)
    x = torch.rand(2, ci, 13, 11, generator=g) * 2 - 1
    w = torch.randn(co, ci, *k, generator=g) / (ci * k[0] * k[1]) ** 0.5
    b = torch.randn(co, generator=g) * 0.1
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), s, p))
    OH, OW = ref.shape[2:]
    ldc, c0 = co + 13, 5
    out = torch.full((2, OH, OW, ldc), SENTINEL, device=DEV)
    _conv(_nhwc(x).to(DEV), w, b, s, p, [(out, ldc, c0, co)], bn=bn)
    got = out.cpu()
    assert torch.all(got[..., :c0] == SENTINEL) and torch.all(got[..., c0 + co:] == SENTINEL)
    err = _rel(got[..., c0:c0 + co].permute(0, 3, 1, 2), ref)
    assert err < 1e-5, err           # one fp32 fma chain over K = kh kw Ci (up to 4 032): measured <= 3.7e-6


def test_fused_heads_route_columns():
    """One GEMM, three 1x1 heads (InceptionE's 320 + 384 + 448) routed to three destinations."""
    g = torch.Generator().manual_seed(5)
    x = torch.rand(3, 64, 8, 8, generator=g) * 2 - 1
    cos = [320, 384, 448]
    ws = [torch.randn(c, 64, 1, 1, generator=g) / 8 for c in cos]
    bs = [torch.randn(c, generator=g) * 0.1 for c in cos]
    outs = [torch.full((3, 8, 8, 2048), SENTINEL, device=DEV), torch.full((3, 8, 8, 384), SENTINEL, device=DEV),
            torch.full((3, 8, 8, 460), SENTINEL, device=DEV)]
    dsts = [(outs[0], 2048, 0, 320), (outs[1], 384, 0, 384), (outs[2], 460, 12, 448)]
    _conv(_nhwc(x).to(DEV), torch.cat(ws), torch.cat(bs), (1, 1), (0, 0), dsts)
    for (t, ldc, c0, nc), w, b in zip(dsts, ws, bs):
        ref = F.relu(F.conv2d(x.double(), w.double(), b.double()))
        got = t.cpu()
        assert _rel(got[..., c0:c0 + nc].permute(0, 3, 1, 2), ref) < 2e-6
        assert torch.all(got[..., :c0] == SENTINEL) and torch.all(got[..., c0 + nc:] == SENTINEL)


def test_pools_and_mean():
    L = _lib()
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 64, 17, 15, generator=g)
    xd = _nhwc(x).to(DEV)
    out = torch.full((2, 8, 7, 100), SENTINEL, device=DEV)
    L.check(L.lib.rick_inc_maxpool_f32(xd.data_ptr(), out.data_ptr(), 2, 17, 15, 64, 100, 20, L.stream_ptr()), 'maxpool')
    ref = F.max_pool2d(x, 3, 2)
    got = out.cpu()
    assert torch.equal(got[..., 20:84].permute(0, 3, 1, 2), ref)
    assert torch.all(got[..., :20] == SENTINEL) and torch.all(got[..., 84:] == SENTINEL)
    avg = torch.empty(2, 17, 15, 64, device=DEV)
    L.check(L.lib.rick_inc_avgpool_f32(xd.data_ptr(), avg.data_ptr(), 2, 17, 15, 64, L.stream_ptr()), 'avgpool')
    ref = F.avg_pool2d(x.double(), 3, 1, 1, count_include_pad=True)
    assert _rel(avg.cpu().permute(0, 3, 1, 2), ref) < 1e-6
    m = torch.empty(2, 64, device=DEV)
    L.check(L.lib.rick_inc_mean_f32(xd.data_ptr(), m.data_ptr(), 2, 17 * 15, 64, L.stream_ptr()), 'mean')
    assert _rel(m.cpu(), x.double().mean((2, 3))) < 1e-6


def _generator_images(n, seed=2, size=256):
    from rick_amd.models import Generator
    from rick_amd.synth import synth_latents, synth_state_dict
    from tests.shapes import generator_shapes
    g = Generator(size, 512, 8, channel_multiplier=2)
    g.load_state_dict(synth_state_dict(generator_shapes(size)), strict=False)
    g = g.to(DEV).eval()
    fwd = g.forward
    g.forward = lambda styles, **kw: fwd(styles, randomize_noise=False, **kw)
    with torch.no_grad():
        img, _ = g([synth_latents(n, seed=seed).to(DEV)])
    return g, img


@pytest.fixture(scope='module')
def gen_images():
    return _generator_images(4)


@pytest.mark.parametrize('dims', [2048, 64, 192, 768])
def test_whole_network_vs_fp64(gen_images, dims):
    from rick_amd.inception import InceptionV3Features
    _, img = gen_images
    sd = synthetic_state_dict(0)
    net = InceptionV3Features.load(sd, device=DEV, dims=dims, batch=4)
    got = net(img)
    assert got.shape == (4, dims) and got.is_cuda
    ref = forward_f64(sd, img.cpu(), dims)
    err = _rel(got, ref)
    print(f'\nwhole network dims {dims}: max |d| / max |f64| = {err:.3e}')
    assert err <= 1e-4, err


def _fixed_generator(size=64):
    from rick_amd.models import Generator
    from rick_amd.synth import synth_state_dict
    from tests.shapes import generator_shapes
    g = Generator(size, 512, 8, channel_multiplier=2)
    g.load_state_dict(synth_state_dict(generator_shapes(size)), strict=False)
    g = g.to(DEV)
    fwd = g.forward
    g.forward = lambda styles, **kw: fwd(styles, randomize_noise=False, **kw)
    return g


def test_fid_inside_evaluator_vs_fp64_features():
    from rick_amd.evaluate import Evaluator, FeatureStats, frechet_distance, sample_images
    from rick_amd.inception import InceptionV3Features
    from rick_amd.synth import synth_latents, synth_reals
    sd = synthetic_state_dict(0)
    net = InceptionV3Features.load(sd, device=DEV, dims=64)
    g = _fixed_generator()
    z = synth_latents(96, seed=11)
    real = synth_reals(96, size=64, seed=4)
    ev = Evaluator(g, net, net(real.to(DEV)), n_sample_store=25, inception_nsamples=96, fid_sample_size=96)
    fid = float(ev.compute_inception_score(fid=True, latents=z)['fid'])
    fake_img, _ = sample_images(g, 96, n_sample_store=25, latents=z)
    fr, ff = forward_f64(sd, real, 64), forward_f64(sd, fake_img.cpu(), 64)
    ref = float(frechet_distance(*FeatureStats(64, 'cpu').update(fr).finalize(), *FeatureStats(64, 'cpu').update(ff).finalize()))
    print(f'\nFID dims 64: HIP {fid:.6f}  fp64 {ref:.6f}  rel {abs(fid - ref) / abs(ref):.3e}')
    assert abs(fid - ref) <= 1e-3 * abs(ref)


def test_evaluator_equals_hand_called_statistics_bitwise():
    from rick_amd.evaluate import Evaluator, FeatureStats, frechet_distance
    from rick_amd.inception import InceptionV3Features
    from rick_amd.synth import synth_latents, synth_reals
    net = InceptionV3Features.load(synthetic_state_dict(0), device=DEV, dims=192)
    g = _fixed_generator()
    z = synth_latents(50, seed=12).to(DEV)
    real = net(synth_reals(60, size=64, seed=5).to(DEV))
    got = Evaluator(g, net, real, n_sample_store=25, inception_nsamples=50, fid_sample_size=50).compute_inception_score(
        fid=True, latents=z)['fid']
    with torch.no_grad():
        fake = torch.cat([net(g([z[i:i + 25]])[0]) for i in range(0, 50, 25)])
    want = frechet_distance(*FeatureStats(192, DEV).update(real).finalize(), *FeatureStats(192, DEV).update(fake).finalize())
    assert torch.equal(got, want)


def test_run_to_run_bit_identical(gen_images):
    from rick_amd.inception import InceptionV3Features
    _, img = gen_images
    net = InceptionV3Features.load(synthetic_state_dict(0), device=DEV, dims=2048, batch=4)
    a, b = net(img), net(img)
    assert torch.equal(a, b)


def test_cuda_graph_replay_equals_eager():
    from rick_amd.inception import InceptionV3Features
    from rick_amd.synth import synth_reals
    net = InceptionV3Features.load(synthetic_state_dict(0), device=DEV, dims=2048, batch=100)
    x = synth_reals(25, size=64, seed=8).to(DEV)
    eager = net(x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        net(x)                                   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = net(x)
    x.copy_(synth_reals(25, size=64, seed=9).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, net(x))
    x.copy_(synth_reals(25, size=64, seed=8).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_chunking_over_the_batch():
    from rick_amd.inception import InceptionV3Features
    from rick_amd.synth import synth_reals
    net = InceptionV3Features.load(synthetic_state_dict(0), device=DEV, dims=2048, batch=100)
    x = synth_reals(250, size=64, seed=10).to(DEV)
    whole = net(x)
    parts = torch.cat([net(x[i:i + 25]) for i in range(0, 250, 25)])
    err = float((whole - parts).abs().max() / parts.abs().max())
    print(f'\nchunking: max |d| / max = {err:.3e}')
    assert err <= 1e-4
