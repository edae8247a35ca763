"""What the kernel-forms tests share (test_gpu_wgrad_forms.py, test_gpu_igemm_forms.py, test_gpu_convt2_forms.py,
test_gpu_ufd_forms.py, test_gpu_mod_forms.py, test_gpu_state_forms.py, test_gpu_gemm_forms.py, test_gpu_ada_forms.py): guarded and fenced device buffers, the integer / 12-bit / scale generators of the exact modes, split images, the saturation counter, the
NaN-fence and amax-word checks, the terms of the a-priori bound.  A plain module: no fixtures, no pytest hooks."""
import ctypes
import math
import zlib

import torch

DEV = 'cuda'
PAD = 64                      # floats of guard band either side (a multiple of 4: the 16-byte alignment is kept)
SENT = -7777.125              # no exact-mode result can equal it (asserted)
AMAX_FLOATS, AMAX_STRIDE = 512, 32        # a running-maximum word: 16 slots, one per 128-byte line (include/rick_hip.h)


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def cdiv(a, b):
    return -(-a // b)


def ilog2_ceil(v):
    l = 0
    while (1 << l) < v:
        l += 1
    return l


# ----------------------------------------------------------------------------------------------------------- inputs
def _gen(key):
    gen = torch.Generator(device='cpu')
    gen.manual_seed(zlib.crc32(key.encode()) & 0x7FFFFFFF)
    return gen


def ints(key, shape, amp):
    """Non-zero integers in [-amp, amp] as fp32, both signs."""
    gen = _gen(key)
    mag = torch.randint(1, amp + 1, tuple(shape), generator=gen).float()
    return mag * (torch.randint(0, 2, tuple(shape), generator=gen).float() * 2 - 1)


def fine(key, shape):
    """sign * (k + m * 2**-10), k in {2, 3}, m in {1, 3}: |v| in (2, 4) with the 12th significant bit set — fp16 cannot hold it."""
    gen = _gen(key)
    k = torch.randint(2, 4, tuple(shape), generator=gen).float()
    m = torch.randint(0, 2, tuple(shape), generator=gen).float() * 2 + 1
    v = (k + m * 2.0 ** -10) * (torch.randint(0, 2, tuple(shape), generator=gen).float() * 2 - 1)
    assert bool((v.half().float() != v).all())
    return v


def scales(key, shape, mode):
    gen = _gen(key)
    if mode == 'bound':
        return 0.5 + torch.rand(tuple(shape), generator=gen)
    return torch.pow(2.0, torch.randint(-1, 2, tuple(shape), generator=gen).float())


# ----------------------------------------------------------------------------------------------------- device helpers
class Guarded:
    """numel floats between two sentinel bands (`off` floats of extra offset misalign them: a slice of a flat buffer)."""

    def __init__(self, numel, src=None, off=0):
        self.buf = torch.full((PAD + off + numel + PAD,), SENT, device=DEV, dtype=torch.float32)
        self.lo, self.hi = PAD + off, PAD + off + numel
        self.v = self.buf[self.lo:self.hi]
        assert self.v.data_ptr() % 16 == 4 * (off % 4)
        if src is not None:
            self.v.copy_(src.reshape(-1))

    def assert_bands(self, what):
        assert bool((self.buf[:self.lo] == SENT).all()) and bool((self.buf[self.hi:] == SENT).all()), f'{what}: wrote outside its buffer'

    def untouched(self):
        return bool((self.buf == SENT).all())


class Fenced:
    """An operand as a view into a larger buffer with NaN on both sides (`off` floats of extra offset misalign it): a read
    outside the operand but inside the allocation poisons the result.  image = True: the fence is NaN as fp16 halves; `fill`:
    another fence value, for operands that only pass through fmaxf (which drops a NaN: +inf there)."""

    def __init__(self, numel, src=None, off=0, image=False, fill=float('nan')):
        n4 = cdiv(numel, 4) * 4
        if image:
            self.buf = torch.full((PAD + off + n4 + PAD,), 0x7E007E00, device=DEV, dtype=torch.int32).view(torch.float32)
        else:
            self.buf = torch.full((PAD + off + n4 + PAD,), fill, device=DEV, dtype=torch.float32)
        self.v = self.buf[PAD + off:PAD + off + numel]
        assert self.v.data_ptr() % 16 == 4 * (off % 4)
        if src is not None:
            self.v.copy_(src.reshape(-1))


def p(gd):
    return None if gd is None else gd.v.data_ptr()


def fenced(tn, off=0, fill=float('nan')):
    return None if tn is None else Fenced(tn.numel(), tn, off, fill=fill)


def stream():
    from rick_amd._lib import stream_ptr
    return stream_ptr()


def sat_count():
    from rick_amd._lib import check, lib
    cnt = ctypes.c_uint(0)
    check(lib.rick_saturation_count(ctypes.byref(cnt), 0), 'rick_saturation_count')
    return cnt.value


def nan_fence_ok(fd):
    """The bands of a Fenced buffer still hold what they were filled with (a view the device writes: the packed weight)."""
    n = fd.buf.numel() - fd.v.numel()
    lo = fd.v.data_ptr() - fd.buf.data_ptr() >> 2
    bits = fd.buf.view(torch.int32)
    want = bits[0].item()
    return bool((bits[:lo] == want).all()) and bool((bits[lo + fd.v.numel():] == want).all()) and n > 0


def amax_word_check(word, expect, what):
    """An amax word (a CPU tensor of AMAX_FLOATS): the maximum over its 16 slots is `expect` exactly, nothing lies between them."""
    slots = word[::AMAX_STRIDE]
    assert float(slots.max()) == expect, f'{what}: amax word {float(slots.max())} != max |out| {expect}'
    rest = word.clone()
    rest[::AMAX_STRIDE] = 0
    assert not bool(rest.any()), f'{what}: amax word written between its slots'


# ----------------------------------------------------------------------------------------------- the a-priori bound
def rep_of(split):
    """Representation: |v - hi - lo| <= 2**-22 |v| on either operand and the dropped lo*lo; plain fp16: 2**-11 on either."""
    return 3 * 2.0 ** -22 if split == 2 else 2 * 2.0 ** -11


def bound_terms(S, wn, add, K, R, rep):
    """Representation, values below the exponent window, and fp32 accumulation of K terms with R further roundings, on
    S = sum |terms| (+ `add`: what a tail adds); the callers add the partial sums of split-K and one ulp of the result."""
    return rep * S + 2.0 ** -27 * wn + (K + R) * 2.0 ** -24 * (S + add)


def split_halves(v, lo=True):
    """The documented split on the CPU with ONE exponent for the tensor (maximum placed in [4, 8), as CV_EXP_TARGET = 2):
    hi = fp16(v * 2^e), lo = fp16(v * 2^e - hi) (zero with lo = False) -> (hi, lo, 2^-e), fp64."""
    e = 2 - math.floor(math.log2(float(v.abs().max())))
    w = v.float() * 2.0 ** e
    hi = w.half()
    lw = (w - hi.float()).half() if lo else torch.zeros_like(hi)
    return hi.double(), lw.double(), 2.0 ** -e


def decode_image(img, hdr):
    """A split image (CPU, viewed as fp32) and its header -> the values it holds, (hi + lo) * 2^-e, flat."""
    h = img.view(torch.float16).reshape(-1, 8).float()
    return ((h[:, :4] + h[:, 4:]) * hdr[1]).reshape(-1)


def split_image(tn):
    """rick_split_pack_f32 of an fp32 tensor under its exact maximum -> (image, header), both fenced."""
    from rick_amd._lib import lib
    word = torch.zeros(AMAX_FLOATS)
    word[3 * AMAX_STRIDE] = float(tn.abs().max())
    src, wd = fenced(tn), fenced(word)
    img, hdr = Fenced(tn.numel(), image=True), Fenced(4)
    assert lib.rick_split_pack_f32(p(src), p(img), p(hdr), p(wd), None, 1.0, tn.numel() // tn.shape[-1], tn.shape[-1], stream()) == 0
    torch.cuda.synchronize()
    return img, hdr
