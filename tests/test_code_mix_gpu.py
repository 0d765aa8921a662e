"""isi_embed_mix_f32 (csrc/code_mix.hip) against its float64 specification (tests/code_mix_spec.py, which also holds the
test data and the comparison), and the public path above it -- VQVAE.decode_code_mix, inpainting.morph / morph_sweep /
crossfade -- against decode_code on the cases where a mixture IS a codemap.

Kernel cases: D in {4, 12, 64} (1, 3 and 16 lanes per cell: with 3, cells straddle waves and workgroups), N in {1, 17, 257,
1031}, M in {1, 2, 3, 8}, K in {1, 3, 512}, every one with ids_stride, w_stride and ldo larger than needed and unrelated,
the output inside a buffer of a NaN no kernel makes.  Bound: T 2^-24 sum |w e| (1 + 2^-20) for a cell of T terms, nothing
looser; NaN cells, empty cells and weight-1 cells are compared bit for bit (code_mix_spec.compare).

The end-to-end cases use the seeded default model of tests/test_code_tables_gpu.py (oracle seed 4, calibration generator
seed 9) and the map sizes of a [1, 2, 64, 128] input.  One thing differs: the calibration batch has 4 samples instead of
2.  With 2 the top level offers 256 vectors for 512 codes, the oracle then draws rows with replacement and the top codebook
has 226 distinct rows -- the premise asserted below (pairwise distinct rows, which `snap` needs to give a code back) would
not hold.  With 4 samples both levels pick 512 well-separated rows.

A recording aid, not a check: with ISI_CODE_MIX_RECORD=<file> in the environment the worst error / bound ratio of every
kernel case is written there when the module ends (profiles/code_mix_checks.txt is such a run on an MI355X)."""
import os

import pytest
import torch

import code_mix_spec as S

pytestmark = pytest.mark.gpu

RECORD = []      # (ratio, case name)
GUARD = 16       # floats of poison in front of and behind an output buffer


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("ISI_CODE_MIX_RECORD")
    if not path or not RECORD:
        return
    with open(path, "w") as f:
        f.write("# worst error / bound of isi_embed_mix_f32 against the float64 spec, per case of tests/test_code_mix_gpu.py; bound:\n"
                "# T 2^-24 sum |w e| (1 + 2^-20) per cell of T terms (tests/code_mix_spec.py).  Worst first; 'exact': bit for bit.\n")
        for ratio, what in sorted(RECORD, key=lambda r: -r[0]):
            f.write(f"{ratio:8.3f}  {what}\n" if ratio > 0 else f"   exact  {what}\n")


def _launch(ids_buf, ids_stride, w_buf, w_stride, E, N, M, D, K, ldo):
    """the kernel on host tensors: ([N, D] result, True if the guards and the padding between cells came back untouched)"""
    from interactive_spectrogram_inpainting import _hip
    L, dev = _hip.lib(), _dev()
    ids, w, codes = ids_buf.to(dev), w_buf.to(dev), E.to(dev)
    buf = torch.full((GUARD + N * ldo + GUARD,), S.OUT_POISON, dtype=torch.int32, device=dev)
    out = buf[GUARD:]
    rc = L.isi_embed_mix_f32(ids.data_ptr(), ids_stride, w.data_ptr(), w_stride, codes.data_ptr(), out.data_ptr(), ldo, N, M, D, K,
                             _hip.stream_ptr(dev))
    assert rc == 0, L.isi_last_error()
    torch.cuda.synchronize()
    assert torch.equal(ids.cpu(), ids_buf) and torch.equal(S.bits(w.cpu()), S.bits(w_buf)) and torch.equal(S.bits(codes.cpu()), S.bits(E)), \
        "the kernel changed an input"
    host = buf.cpu()
    cells = host[GUARD:GUARD + N * ldo].reshape(N, ldo)
    clean = bool((host[:GUARD] == S.OUT_POISON).all()) and bool((host[GUARD + N * ldo:] == S.OUT_POISON).all()) and \
        bool((cells[:, D:] == S.OUT_POISON).all())
    return cells[:, :D].contiguous().view(torch.float32), clean


def _run(case):
    return _launch(case.ids_buf, case.ids_stride, case.w_buf, case.w_stride, case.E, case.N, case.M, case.D, case.K, case.ldo)


@pytest.mark.parametrize("N", [1, 17, 257, 1031])
@pytest.mark.parametrize("D", [4, 12, 64])
def test_kernel_against_the_spec(D, N):
    for M in (1, 2, 3, 8):
        for K in (1, 3, 512):
            what = f"D={D} N={N} M={M} K={K}"
            case = S.make_case(N, M, D, K)
            assert case.ids_stride > N and case.w_stride > N and case.ldo > D
            if N >= 17:
                assert len(case.bad_cells) == 3
            got, clean = _run(case)
            assert clean, f"{what}: a write outside the cells"
            ratio = S.compare(got, case, what)
            print(f"{what}: worst error / bound = {ratio:.3f}")
            RECORD.append((ratio, what))


def test_one_hot_weights_equal_embed_code_bit_for_bit():
    from interactive_spectrogram_inpainting import _hip
    L, dev = _hip.lib(), _dev()
    N, M, D, K = 1031, 3, 64, 512
    g = torch.Generator().manual_seed(7)
    E = torch.randn(K, D, generator=g)
    E[torch.rand(K, D, generator=g) < 0.05] = -0.0
    ids = torch.randint(0, K, (M, N), generator=g)
    ids[0, 0], ids[-1, -1] = 0, K - 1
    hot = torch.randint(0, M, (N,), generator=g)
    hot[0], hot[-1] = 0, M - 1
    w = torch.zeros(M, N)
    w[1::2] = -0.0
    w[hot, torch.arange(N)] = 1.0
    chosen = ids[hot, torch.arange(N)].contiguous()
    ids[w == 0] = -1                                         # whatever the other sources hold
    got, clean = _launch(ids.reshape(-1), N, w.reshape(-1), N, E, N, M, D, K, D)
    assert clean
    want = torch.empty(N, D, device=dev)
    assert L.isi_embed_code_f32(chosen.to(dev).data_ptr(), E.to(dev).data_ptr(), want.data_ptr(), N, D, K, _hip.stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    assert torch.equal(S.bits(got), S.bits(want.cpu())) and torch.equal(S.bits(got), S.bits(E[chosen]))
    RECORD.append((0.0, f"one-hot weights against isi_embed_code_f32 D={D} N={N} M={M} K={K}"))


@pytest.mark.parametrize("D,M", [(12, 3), (64, 8)])
def test_integer_codebook_and_power_of_two_weights_are_exact(D, M):
    """every product and every partial sum is an integer multiple of 2^-2 far below 2^24: the fp32 chain rounds nowhere
    and must give the float64 sum's bits, zeros' signs included"""
    N, K = 257, 512
    g = torch.Generator().manual_seed(11 + D)
    E = torch.randint(-64, 65, (K, D), generator=g).float()
    ids = torch.randint(0, K, (M, N), generator=g)
    w = torch.tensor([0.25, 0.5, 1.0, 2.0, -0.5, -1.0, 0.0, -0.0])[torch.randint(0, 8, (M, N), generator=g)]
    if M >= 2:
        ids[1, ::5], w[1, ::5] = ids[0, ::5], -w[0, ::5]     # exact cancellations: +0.0, or -0.0 where nothing else exists
    got, clean = _launch(ids.reshape(-1), N, w.reshape(-1), N, E, N, M, D, K, D)
    mix, _, _, bad = S.mix_spec(ids, w, E)
    assert clean and not bad.any()
    assert torch.equal(S.bits(got), S.bits(mix.float()))
    RECORD.append((0.0, f"integer codebook, power-of-two weights D={D} N={N} M={M} K={K}"))


def test_a_cell_does_not_depend_on_the_launch():
    """the same 257 cells alone and as the head of 1031 cells (other strides, other workgroup boundaries)"""
    D, M, K = 12, 3, 512
    small, big = S.make_case(257, M, D, K), S.make_case(1031, M, D, K, seed=1)
    ids, w = big.ids.clone(), big.weights.clone()
    ids[:, :257], w[:, :257] = small.ids, small.weights
    a, clean_a = _run(small)
    b, clean_b = _launch(ids.reshape(-1), 1031, w.reshape(-1), 1031, small.E, 1031, M, D, K, D)
    assert clean_a and clean_b
    assert torch.equal(S.bits(a), S.bits(b[:257]))
    RECORD.append((0.0, f"the same cells at N=257 and N=1031 D={D} M={M} K={K}"))


# ------------------------------------------------------------------------------------------------------- end to end
class _Model:
    def __init__(self):
        from oracle import vqvae_oracle as O
        from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
        cfg = O.Config(in_channel=2)
        sd = O.init_state_dict(cfg, seed=4)
        O.calibrate_codebooks(sd, cfg, torch.randn(4, 2, 64, 128, generator=torch.Generator().manual_seed(9)))
        tiny = torch.finfo(torch.float32).tiny
        for level in ("t", "b"):                              # on the CPU: the premises of the bit-for-bit cases
            e = sd[f"quantize_{level}.embed"].t()
            assert torch.unique(e, dim=0).shape[0] == e.shape[0], f"codebook {level}: rows are not pairwise distinct"
            assert not bool(((e != 0) & (e.abs() < tiny)).any()), f"codebook {level}: subnormal entries"
        m = VQVAE(in_channel=2)
        m.load_state_dict(sd)
        self.m = m.to(_dev()).eval()
        self.K = cfg.num_embeddings
        Hb, Wb, Ht, Wt, _ = self.m._latent_shapes(64, 128)
        self.top, self.bottom = (1, Ht, Wt), (1, Hb, Wb)

    def sound(self, seed):
        g = torch.Generator().manual_seed(seed)
        top, bottom = torch.randint(0, self.K, self.top, generator=g), torch.randint(0, self.K, self.bottom, generator=g)
        top[0, 0, 0], bottom[0, -1, -1] = 0, self.K - 1
        return top.to(_dev()), bottom.to(_dev())


@pytest.fixture(scope="module")
def model():
    return _Model()


class _DecodeInputs:
    """records the maps that reach VQVAE.decode while the block runs"""

    def __init__(self, m):
        self.m, self.seen = m, []

    def __enter__(self):
        inner = self.m.decode

        def decode(quant_t, quant_b):
            self.seen.append((quant_t.clone(), quant_b.clone()))
            return inner(quant_t, quant_b)
        self.m.decode = decode
        return self

    def __exit__(self, *exc):
        del self.m.decode
        return False


def _ones(*maps):
    return [torch.ones(1, *c.shape, device=c.device) for c in maps]


def test_one_source_of_weight_one_is_decode_code(model):
    m = model.m
    top, bottom = model.sound(1)
    w_t, w_b = _ones(top, bottom)
    with _DecodeInputs(m) as rec:
        got = m.decode_code_mix(top[None], w_t, bottom[None], w_b)
    quant_t, quant_b = rec.seen[0]
    assert quant_t.permute(0, 2, 3, 1).is_contiguous() and quant_b.permute(0, 2, 3, 1).is_contiguous(), \
        "the mixed maps reach decode in channels-last storage: no copy"
    assert torch.equal(got, m.decode_code(top, bottom))


def test_one_hot_maps_and_the_hard_cut_are_decode_code_of_the_splice(model):
    import inpainting
    m = model.m
    a, b = model.sound(2), model.sound(3)
    cut = 5                                                   # a left of top column 5, b from it on
    ratio = b[1].shape[-1] // b[0].shape[-1]
    top = torch.cat([a[0][..., :cut], b[0][..., cut:]], -1)
    bottom = torch.cat([a[1][..., :ratio * cut], b[1][..., ratio * cut:]], -1)
    want = m.decode_code(top, bottom)
    take_b_t = (torch.arange(top.shape[-1], device=_dev()) >= cut).float().expand(top.shape)
    take_b_b = (torch.arange(bottom.shape[-1], device=_dev()) >= ratio * cut).float().expand(bottom.shape)
    got = m.decode_code_mix(torch.stack([a[0], b[0]]), torch.stack([1 - take_b_t, take_b_t]),
                            torch.stack([a[1], b[1]]), torch.stack([1 - take_b_b, take_b_b]))
    assert torch.equal(got, want)
    assert torch.equal(inpainting.crossfade(m, a, b, cut, 0), want)
    assert torch.equal(inpainting.morph(m, [a, b], torch.stack([1 - take_b_t[0, 0], take_b_t[0, 0]])), want)


def test_half_and_half_is_the_decode_of_torch_s_blend(model):
    """0.5 e is exact (no subnormals), so the kernel's fma chain and torch's 0.5 * qa + 0.5 * qb both round once"""
    import inpainting
    m = model.m
    a, b = model.sound(4), model.sound(5)
    blend = [0.5 * q.embed_code(ca).permute(0, 3, 1, 2) + 0.5 * q.embed_code(cb).permute(0, 3, 1, 2)
             for q, ca, cb in ((m.quantize_t, a[0], b[0]), (m.quantize_b, a[1], b[1]))]
    assert torch.equal(inpainting.morph(m, [a, b], [0.5, 0.5]), m.decode(*blend))


def test_sweep_rows_are_single_morphs(model):
    import inpainting
    m = model.m
    a, b = model.sound(6), model.sound(7)
    steps = 5
    with _DecodeInputs(m) as rec:
        sweep = inpainting.morph_sweep(m, a, b, steps)
    assert len(rec.seen) == 1, "one batch, one decode call"
    sweep_t, sweep_b = rec.seen[0]
    assert sweep.shape[0] == sweep_t.shape[0] == sweep_b.shape[0] == steps
    alpha = torch.linspace(0, 1, steps)
    for s in range(steps):
        with _DecodeInputs(m) as rec:
            inpainting.morph(m, [a, b], [float(1 - alpha[s]), float(alpha[s])])
        one_t, one_b = rec.seen[0]
        assert torch.equal(S.bits(sweep_t[s:s + 1]), S.bits(one_t)) and torch.equal(S.bits(sweep_b[s:s + 1]), S.bits(one_b)), f"row {s}"
    assert torch.equal(sweep[:1], m.decode_code(*a)) and torch.equal(sweep[-1:], m.decode_code(*b))


def test_snap_returns_codes(model):
    import inpainting
    m = model.m
    a, b = model.sound(8), model.sound(9)
    cut = 9
    ratio = b[1].shape[-1] // b[0].shape[-1]
    top, bottom = inpainting.crossfade(m, a, b, cut, 0, snap=True)      # one-hot weights: the sources' own codes
    assert torch.equal(top, torch.cat([a[0][..., :cut], b[0][..., cut:]], -1))
    assert torch.equal(bottom, torch.cat([a[1][..., :ratio * cut], b[1][..., ratio * cut:]], -1))
    top, bottom = inpainting.morph(m, [a, b], [0.5, 0.5], snap=True)
    assert top.shape == a[0].shape and bottom.shape == a[1].shape and top.dtype == bottom.dtype == torch.int64
    for codes in (top, bottom):
        assert int(codes.min()) >= 0 and int(codes.max()) < model.K
    assert not m.quantize_t.training and not m.quantize_b.training
