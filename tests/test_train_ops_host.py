"""CPU-side half of the checks of the VQ-VAE training step's small kernels (tests/test_train_ops_gpu.py holds the kernels
themselves): the closed-form float64 specifications of tests/tests_support.py equal float64 autograd of the reference
formulation; `compare_rows` or bit equality rejects, applied to the float32 torch evaluation of each operation, every fault
a GPU case exists to catch; the C-ABI refuses, before any launch, the arguments the kernels are not laid out for; the
path-choosing helpers give the counts the GPU cases rely on."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import tests_support as TS

CAP = TS.TRAIN_OPS_GRID_CAP        # 8192 blocks of 256 threads: one float4 each in the first pass of a grid-stride loop


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _rejected(got, ref, yardstick, what):
    with pytest.raises(AssertionError, match=what):
        TS.compare_rows(got, ref, yardstick, what)


# ----------------------------------------------------------------------------------- the specs against float64 autograd
@pytest.mark.parametrize("M,D,g", [(1, 4, 0.25), (7, 8, 0.25), (33, 64, 0.0)])
def test_vq_bwd_spec_equals_float64_autograd_of_straight_through_and_commitment(M, D, g):
    gen = torch.Generator().manual_seed(10 + M)
    z, q, dq = (torch.randn(M, D, generator=gen) for _ in range(3))
    zd = z.double().requires_grad_(True)
    qd = q.double()
    quantize = zd + (qd - zd).detach()                   # bottleneck.py:95
    diff = (qd.detach() - zd).pow(2).mean()              # bottleneck.py:94
    ((quantize * dq.double()).sum() + g * diff).backward()
    q_st = z.double() + (qd - z.double())                # what the forward stored
    assert _rel(TS.vq_bwd_spec(dq, z.double(), q_st, g), zd.grad) <= 1e-12
    # a row-strided dq gives the same values
    wide = torch.full((M, D + 4), float("nan"))
    wide[:, :D] = dq
    assert torch.equal(TS.vq_bwd_spec(wide[:, :D], z, q, g), TS.vq_bwd_spec(dq, z, q, g))


@pytest.mark.parametrize("n", [1, 5, 1027])
def test_mse_spec_equals_float64_autograd_of_mse_loss(n):
    gen = torch.Generator().manual_seed(20 + n)
    a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    ad, bd = a.double().requires_grad_(True), b.double().requires_grad_(True)
    loss = F.mse_loss(ad, bd)
    (loss * 0.75).backward()
    value, da, db = TS.mse_spec(a, b, 0.75)
    assert value.shape == (1,) and abs(float(value) - float(loss.detach())) <= 1e-12 * float(loss.detach())
    assert _rel(da, ad.grad) <= 1e-12 and _rel(db, bd.grad) <= 1e-12


def test_relu_gates_equal_float64_autograd_of_relu():
    gen = torch.Generator().manual_seed(30)
    x = torch.randn(9, 12, generator=gen)
    x[0, :4] = torch.tensor([0.0, -0.0, 2.0 ** -126, -2.0 ** -126])
    a, b = torch.randn(9, 12, generator=gen), torch.randn(9, 12, generator=gen)
    xd = x.double().requires_grad_(True)
    y = F.relu(xd)
    (y * a.double()).sum().backward()
    assert torch.equal(TS.relu_bwd_spec(a, y.detach()), xd.grad)
    assert torch.equal(TS.add_gate_rows_spec(a, None, y.detach()), xd.grad)
    xd.grad = None
    y = F.relu(xd)
    ((y * a.double()).sum() + (y * b.double()).sum()).backward()      # two consumers of one rectified tensor
    assert _rel(TS.add_gate_rows_spec(a, b, y.detach()), xd.grad) <= 1e-15
    assert torch.equal(TS.add_gate_rows_spec(a, b, None), a.double() + b.double())
    assert torch.equal(TS.add_gate_rows_spec(a), a.double())
    # a selection: what sits at a masked place does not matter, and both zeros mask
    dy, yv = TS.gate_data(40, gen)
    assert not torch.isfinite(dy).all() and torch.isfinite(TS.relu_bwd_spec(dy, yv)).all()
    assert float(TS.relu_bwd_spec(torch.ones(2), torch.tensor([0.0, -0.0])).abs().sum()) == 0.0
    assert torch.equal(TS.relu_inplace_spec(x), F.relu(x.double()))


@pytest.mark.parametrize("B,Cc,H,W", [(1, 1, 1, 1), (2, 3, 5, 7), (2, 64, 3, 5)])
def test_colsum_spec_equals_the_bias_gradient_of_a_1x1_convolution(B, Cc, H, W):
    gen = torch.Generator().manual_seed(40 + Cc)
    x = torch.randn(B, 5, H, W, generator=gen).double()
    w = torch.randn(Cc, 5, 1, 1, generator=gen).double()
    bias = torch.zeros(Cc, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(B, Cc, H, W, generator=gen)
    (F.conv2d(x, w, bias) * dy.double()).sum().backward()
    assert _rel(TS.colsum_spec(dy.permute(0, 2, 3, 1).reshape(-1, Cc)), bias.grad) <= 1e-12


@pytest.mark.parametrize("D,K", [(8, 32), (16, 1500)])
def test_ema_update_spec_equals_the_oracle_in_float64(D, K):
    from oracle import vqvae_oracle as O
    gen = torch.Generator().manual_seed(50 + K)
    embed, cs, ea, _, _ = TS.ema_state(D, K, gen)
    flat = torch.randn(300, D, generator=gen)
    ind = torch.randint(0, K - 1, (300,), generator=gen)              # (the last code is never drawn)
    decay, eps = float(torch.tensor(0.99)), float(torch.tensor(1e-5))          # the float32 values the C-ABI receives
    want = O.ema_update(flat.double(), ind, embed.double(), cs.double(), ea.double(), decay, eps)
    counts = torch.bincount(ind, minlength=K)
    got = TS.ema_update_spec(embed, cs, ea, counts, TS.embed_sum_spec(flat, ind, K), 0.99, 1e-5)
    assert (counts == 0).any()
    for g, w in zip(got, want):
        assert g.shape == w.shape and _rel(g, w) <= 1e-12


def test_vq_finalize_and_embed_code_specs_equal_the_oracle_in_float64():
    from oracle import vqvae_oracle as O
    gen = torch.Generator().manual_seed(60)
    D, K, N = 8, 137, 150
    embed = torch.randn(D, K, generator=gen).double()
    z = torch.randn(N, D, generator=gen).double()
    _, diff, ind, perplexity = O.quantize(z, embed)
    q = O.embed_code(ind, embed)
    assert torch.equal(TS.embed_code_spec(ind, embed.t(), K), q.reshape(N, D))
    sse_part = (q - z).pow(2).sum(dim=1).reshape(3, 50).sum(dim=1)
    counts = torch.bincount(ind, minlength=K)
    assert (counts == 0).any(), "the clamp must matter"
    got = TS.vq_finalize_spec(sse_part, counts, N, D)
    assert abs(float(got[0]) - float(diff)) <= 1e-12 * float(diff)
    assert abs(float(got[1]) - float(perplexity)) <= 1e-12 * float(perplexity)
    # the documented clamp of out-of-range indices
    codes = embed.t()
    assert torch.equal(TS.embed_code_spec(torch.tensor([-1, K, 2 ** 40, 3]), codes, K), codes[[0, K - 1, K - 1, 3]])


def test_float32_evaluations_pass_their_own_comparison():
    """Every yardstick is accepted against its spec (ratio 1 or the floor), so a rejection below is the mutant's."""
    gen = torch.Generator().manual_seed(70)
    a, b, z = (torch.randn(37, 64, generator=gen) for _ in range(3))
    TS.compare_rows(TS.axpy_f32(a, b, -0.5), TS.axpy_spec(a, b, -0.5), TS.axpy_f32(a, b, -0.5), "axpy")
    TS.compare_rows(TS.vq_bwd_f32(a, z, b, 0.25), TS.vq_bwd_spec(a, z, b, 0.25), TS.vq_bwd_f32(a, z, b, 0.25), "vq_bwd")
    TS.compare_rows(TS.colsum_f32(a + 100), TS.colsum_spec(a + 100), TS.colsum_f32(a + 100), "colsum")
    for got, ref in zip(TS.mse_f32(a, b, 0.75), TS.mse_spec(a, b, 0.75)):
        TS.compare_rows(got, ref, got, "mse")
    dy, y = TS.gate_data(1025, gen)
    assert TS.same_bits(TS.relu_bwd_f32(dy, y), TS.relu_bwd_spec(dy, y))
    assert not TS.same_bits(torch.tensor([0.0]), torch.tensor([-0.0])) and TS.same_bits(torch.tensor([float("nan")]), torch.tensor([float("nan")]))


# ------------------------------------------------------------------------------------------------------------- mutants
@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 1023, 1025])
def test_rejects_an_untouched_vector_tail(n):
    """The last n % 4 elements left as they were: relu_bwd's in-place operand keeps dy (bit equality), the MSE gradients
    keep their NaN fill and the MSE value misses the tail's squares."""
    gen = torch.Generator().manual_seed(100 + n)
    dy, y = TS.gate_data(n, gen)
    dy[n - 1], y[n - 1] = 1.25, -1.0                       # the last element is masked and finite
    got = TS.relu_bwd_f32(dy, y)
    assert TS.same_bits(got, TS.relu_bwd_spec(dy, y))
    got[n - n % 4:] = dy[n - n % 4:]
    assert not TS.same_bits(got, TS.relu_bwd_spec(dy, y))
    a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    ref, yard = TS.mse_spec(a, b, 0.75), TS.mse_f32(a, b, 0.75)
    _rejected(TS.mse_f32(a, b, 0.75, count=n - n % 4)[0], ref[0], yard[0], "value")
    for i, name in ((1, "da"), (2, "db")):
        got = yard[i].clone()
        got[n - n % 4:] = float("nan")
        _rejected(got, ref[i], yard[i], name)


def test_rejects_a_grid_stride_loop_that_runs_once():
    """Everything past the first 8192 x 256 float4 left untouched, at the past-cap lengths of the GPU tests: in-place
    operands keep their contents, outputs their NaN fill, the MSE value (capped at 1024 x 256 float4) loses the rest."""
    gen = torch.Generator().manual_seed(110)
    n = 4 * CAP + 1203
    dy, y = TS.gate_data(n, gen)
    dy[4 * CAP + 8], y[4 * CAP + 8] = 1.25, -1.0
    got = TS.relu_bwd_f32(dy, y)
    got[4 * CAP:] = dy[4 * CAP:]
    assert not TS.same_bits(got, TS.relu_bwd_spec(dy, y))
    n, M, Cc = 4 * CAP + 1200, 65600, 128                  # M x Cc: the row kernels' case, 2 099 200 float4
    a2, b2, z = (torch.randn(M * Cc, generator=gen) for _ in range(3))
    a, b, z = a2[:n], b2[:n], z[:n]
    yard = TS.axpy_f32(a, b, -0.5)
    got = yard.clone()
    got[4 * CAP:] = a[4 * CAP:]
    _rejected(got, TS.axpy_spec(a, b, -0.5), yard, "axpy")
    yard = TS.vq_bwd_f32(a, z, b, 0.25)
    got = yard.clone()
    got[4 * CAP:] = float("nan")
    _rejected(got, TS.vq_bwd_spec(a, z, b, 0.25), yard, "vq_bwd")
    assert M * Cc // 4 > CAP
    a2, b2 = a2.reshape(M, Cc), b2.reshape(M, Cc)
    yard = TS.add_gate_rows_f32(a2, b2)
    got = yard.clone()
    got.reshape(-1)[4 * CAP:] = float("nan")
    _rejected(got, TS.add_gate_rows_spec(a2, b2), yard, "add_gate_rows")
    n = 4 * 1024 * 256 + 1203                              # the MSE forward's cap
    ref, yard = TS.mse_spec(a[:n], b[:n], 0.75), TS.mse_f32(a[:n], b[:n], 0.75)
    _rejected(TS.mse_f32(a[:n], b[:n], 0.75, count=4 * 1024 * 256)[0], ref[0], yard[0], "value")
    x = torch.randn(4096 * 256 + 77, generator=gen)        # relu_inplace: 4096 blocks of scalars
    got = TS.relu_inplace_spec(x).float()
    got[4096 * 256:] = x[4096 * 256:]
    assert not TS.same_bits(got, TS.relu_inplace_spec(x))
    x = torch.randn(8 * CAP + 2400, generator=gen)         # the pair round trip: 8192 x 256 groups of 8
    want = TS.pair_round_f16(x)
    got = want.clone()
    got[8 * CAP:] = x[8 * CAP:]                            # (the decoded tensor keeps what it held: here the unrounded input)
    assert not TS.same_bits(got, want) and TS.same_bits(want.clone(), want)


@pytest.mark.parametrize("M,Cc,ld", [(3, 8, 12), (257, 64, 128), (5, 128, 192)])
def test_rejects_an_ignored_row_stride(M, Cc, ld):
    """lda / ldq / x_stride read as C: the rows are taken from the flat buffer back to back."""
    gen = torch.Generator().manual_seed(120 + M)
    wide = torch.randn(M, ld, generator=gen)
    a = wide[:, :Cc]
    dense = wide.reshape(-1)[:M * Cc].reshape(M, Cc)       # what a kernel that ignores the stride reads
    b, z = torch.randn(M, Cc, generator=gen), torch.randn(M, Cc, generator=gen)
    _rejected(TS.add_gate_rows_f32(dense, b), TS.add_gate_rows_spec(a, b), TS.add_gate_rows_f32(a, b), "add_gate_rows")
    assert not TS.same_bits(TS.add_gate_rows_f32(dense), TS.add_gate_rows_spec(a))
    _rejected(TS.vq_bwd_f32(dense, z, b, 0.25), TS.vq_bwd_spec(a, z, b, 0.25), TS.vq_bwd_f32(a, z, b, 0.25), "vq_bwd_rows")
    _rejected(TS.colsum_f32(dense), TS.colsum_spec(a), TS.colsum_f32(a), "colsum")


@pytest.mark.parametrize("n", [4, 8, 1028])
def test_rejects_the_coefficient_one_over_n(n):
    gen = torch.Generator().manual_seed(130 + n)
    dq, z, q, a, b = (torch.randn(n, generator=gen) for _ in range(5))
    _rejected(TS.vq_bwd_f32(dq, z, q, 0.25, two=1.0), TS.vq_bwd_spec(dq, z, q, 0.25), TS.vq_bwd_f32(dq, z, q, 0.25), "vq_bwd")
    ref, yard, got = TS.mse_spec(a, b, 0.75), TS.mse_f32(a, b, 0.75), TS.mse_f32(a, b, 0.75, two=1.0)
    _rejected(got[1], ref[1], yard[1], "da")
    _rejected(got[2], ref[2], yard[2], "db")
    # with g_diff = 0 the commitment term is gone: the two coincide, which is why the GPU cases run 0.25 as well
    assert torch.equal(TS.vq_bwd_f32(dq, z, q, 0.0, two=1.0), TS.vq_bwd_f32(dq, z, q, 0.0))


@pytest.mark.parametrize("mutant", ["gate_ge", "multiply"])
def test_rejects_the_wrong_gate(mutant):
    """y >= 0 lets +0.0 and -0.0 through; a multiplication by the mask turns a masked NaN or inf into NaN."""
    gen = torch.Generator().manual_seed(140)
    M, Cc = 5, 8
    dy, y = TS.gate_data(M * Cc, gen)
    if mutant == "gate_ge":
        dy = torch.where(torch.isfinite(dy), dy, torch.ones_like(dy))          # (the zeros alone must show it)
    assert not TS.same_bits(TS.relu_bwd_f32(dy, y, **{mutant: True}), TS.relu_bwd_spec(dy, y))
    a, b, y2 = dy.reshape(M, Cc), torch.randn(M, Cc, generator=gen), y.reshape(M, Cc)
    assert not TS.same_bits(TS.add_gate_rows_f32(a, None, y2, **{mutant: True}), TS.add_gate_rows_spec(a, None, y2))
    _rejected(TS.add_gate_rows_f32(a, b, y2, **{mutant: True}), TS.add_gate_rows_spec(a, b, y2), TS.add_gate_rows_f32(a, b, y2),
              "add_gate_rows")


@pytest.mark.parametrize("M,Cc,kind", [(4, 1, "randn"), (2, 2, "randn"), (256, 2, "offset"), (65536, 1, "randn")])
def test_rejects_narrow_columns_folded_as_four(M, Cc, kind):
    gen = torch.Generator().manual_seed(150 + M)
    x = torch.randn(M, Cc, generator=gen) + (100.0 if kind == "offset" else 0.0)
    _rejected(TS.colsum_f32(x, fold4=True), TS.colsum_spec(x), TS.colsum_f32(x), "colsum")


@pytest.mark.parametrize("M,Cc,kind", [(257, 64, "randn"), (65537, 4, "offset"), (70001, 3, "randn"), (70001, 1, "offset")])
def test_rejects_a_column_sum_without_the_last_blocks_rows(M, Cc, kind):
    from interactive_spectrogram_inpainting import _hip
    gen = torch.Generator().manual_seed(160 + M)
    x = torch.randn(M, Cc, generator=gen) + (100.0 if kind == "offset" else 0.0)
    nblk = _hip.lib().isi_colsum_num_partials(M)
    rows = (M + nblk - 1) // nblk                          # a block's share of rows (more than 256 past the cap)
    last = (M - 1) // rows * rows
    assert 0 < last < M
    _rejected(TS.colsum_f32(x, rows=last), TS.colsum_spec(x), TS.colsum_f32(x), "colsum")


@pytest.mark.parametrize("D,K", [(16, 1500), (64, 2048)])
def test_rejects_an_ema_total_over_the_first_1024_codes(D, K):
    gen = torch.Generator().manual_seed(170 + K)
    state = TS.ema_state(D, K, gen)
    ref, yard = TS.ema_update_spec(*state, 0.99, 1e-5), TS.ema_update_f32(*state, 0.99, 1e-5)
    got = TS.ema_update_f32(*state, 0.99, 1e-5, n_codes=1024)
    TS.compare_rows(yard[0], ref[0], yard[0], "embed")
    _rejected(got[0], ref[0], yard[0], "embed")
    # for K <= 1024 the mutant is the operation itself: the GPU cases above 1024 are the ones that see it
    small = TS.ema_state(8, 32, gen)
    assert torch.equal(TS.ema_update_f32(*small, 0.99, 1e-5, n_codes=1024)[0], TS.ema_update_f32(*small, 0.99, 1e-5)[0])


def test_rejects_the_perplexity_without_the_clamp():
    gen = torch.Generator().manual_seed(180)
    K, N, D = 256, 37, 64
    counts = torch.bincount(torch.randint(0, K, (N,), generator=gen), minlength=K)
    sse = torch.rand(257, generator=gen)
    ref, yard = TS.vq_finalize_spec(sse, counts, N, D), TS.vq_finalize_f32(sse, counts, N, D)
    TS.compare_rows(yard[1], ref[1], yard[1], "perplexity")
    _rejected(TS.vq_finalize_f32(sse, counts, N, D, clamp=False)[1], ref[1], yard[1], "perplexity")


# ------------------------------------------------------------------------------------------ refusals before any launch
def test_train_ops_refuse_bad_arguments_before_any_launch():
    from interactive_spectrogram_inpainting import _hip
    L = _hip.lib()
    ok, odd = 0x10000, 0x10004        # non-null, never dereferenced on the host: 16-byte aligned / 4 bytes off
    INVALID = -1

    def refused(rc, message=None):
        assert rc == INVALID
        if message is not None:
            assert message in L.isi_last_error(), L.isi_last_error()

    # relu_bwd
    refused(L.isi_relu_bwd_f32(odd, ok, 8, None), b"relu_bwd: pointers must be 16-byte aligned")
    refused(L.isi_relu_bwd_f32(ok, odd, 8, None), b"relu_bwd: pointers must be 16-byte aligned")
    refused(L.isi_relu_bwd_f32(None, ok, 8, None))
    refused(L.isi_relu_bwd_f32(ok, ok, -1, None))
    assert L.isi_relu_bwd_f32(ok, ok, 0, None) == 0                         # nothing to do: no launch either
    # axpy: n % 4, and (new) alignment
    for n in (1, 6, -4):
        refused(L.isi_axpy_f32(ok, ok, 1.0, n, None), b"axpy: bad argument")
    refused(L.isi_axpy_f32(odd, ok, 1.0, 8, None), b"axpy: pointers must be 16-byte aligned")
    refused(L.isi_axpy_f32(ok, odd, 1.0, 8, None), b"axpy: pointers must be 16-byte aligned")
    refused(L.isi_axpy_f32(ok, None, 1.0, 8, None))
    assert L.isi_axpy_f32(ok, ok, 1.0, 0, None) == 0
    # vq_bwd: n % 4, and (new) alignment of the four float4 operands (g_diff is read as one scalar)
    for n in (0, 2, 1027):
        refused(L.isi_vq_bwd_f32(ok, ok, ok, ok, ok, n, None), b"vq_bwd: bad argument")
    for i in range(4):
        p = [ok] * 4
        p[i] = odd
        refused(L.isi_vq_bwd_f32(*p, ok, 8, None), b"vq_bwd: pointers must be 16-byte aligned")
        p[i] = None
        refused(L.isi_vq_bwd_f32(*p, ok, 8, None), b"vq_bwd: bad argument")
    refused(L.isi_vq_bwd_f32(ok, ok, ok, ok, None, 8, None))
    # vq_bwd_rows: D, ldq multiples of 4, ldq >= D, alignment
    for M, D, ldq in ((3, 6, 8), (3, 8, 10), (3, 8, 4), (0, 8, 8), (3, 0, 8)):
        refused(L.isi_vq_bwd_rows_f32(ok, ok, ldq, ok, ok, ok, M, D, None), b"vq_bwd_rows: bad argument")
    for i in range(4):
        p = [ok] * 4
        p[i] = odd
        refused(L.isi_vq_bwd_rows_f32(p[0], p[1], 8, p[2], p[3], ok, 3, 8, None), b"vq_bwd_rows: pointers must be 16-byte aligned")
    # add_gate_rows: C, lda multiples of 4, lda >= C, alignment of every operand given
    for M, Cc, lda in ((3, 6, 8), (3, 8, 10), (3, 8, 4), (0, 8, 8), (3, 0, 8)):
        refused(L.isi_add_gate_rows_f32(ok, ok, lda, ok, ok, M, Cc, None), b"add_gate_rows: bad argument")
    for i in range(4):
        p = [ok] * 4
        p[i] = odd
        refused(L.isi_add_gate_rows_f32(p[0], p[1], 8, p[2], p[3], 3, 8, None), b"add_gate_rows: pointers must be 16-byte aligned")
    refused(L.isi_add_gate_rows_f32(None, ok, 8, None, None, 3, 8, None))
    # colsum: (new) a row stride below the row
    refused(L.isi_colsum_f32(ok, 7, ok, ok, 3, 8, None), b"colsum: x_stride must be at least C")
    refused(L.isi_colsum_f32(ok, 0, ok, ok, 3, 1, None), b"colsum: x_stride must be at least C")
    for M, Cc in ((0, 8), (3, 0), (-1, 8)):
        refused(L.isi_colsum_f32(ok, 8, ok, ok, M, Cc, None), b"colsum: bad argument")
    for i in range(3):
        p = [ok] * 3
        p[i] = None
        refused(L.isi_colsum_f32(p[0], 8, p[1], p[2], 3, 8, None), b"colsum: bad argument")
    # MSE
    refused(L.isi_mse_loss_f32(odd, ok, 5, ok, ok, None), b"mse_loss: operands must be 16-byte aligned")
    refused(L.isi_mse_loss_f32(ok, odd, 5, ok, ok, None), b"mse_loss: operands must be 16-byte aligned")
    refused(L.isi_mse_loss_f32(ok, ok, 0, ok, ok, None), b"mse_loss: bad argument")
    refused(L.isi_mse_loss_f32(ok, ok, 5, None, ok, None), b"mse_loss: bad argument")
    refused(L.isi_mse_loss_f32(ok, ok, 5, ok, None, None), b"mse_loss: bad argument")
    for i in range(4):
        p = [ok] * 4
        p[i] = odd
        refused(L.isi_mse_loss_bwd_f32(p[0], p[1], ok, 5, p[2], p[3], None), b"mse_loss_bwd: tensors must be 16-byte aligned")
    refused(L.isi_mse_loss_bwd_f32(ok, ok, ok, 5, None, None, None), b"mse_loss_bwd: bad argument")
    refused(L.isi_mse_loss_bwd_f32(ok, ok, None, 5, ok, ok, None), b"mse_loss_bwd: bad argument")
    refused(L.isi_mse_loss_bwd_f32(ok, ok, ok, 0, ok, ok, None), b"mse_loss_bwd: bad argument")
    # vq_finalize, vq_ema_update
    for n_part, K, N, D in ((0, 8, 8, 8), (1, 0, 8, 8), (1, 8, 0, 8), (1, 8, 8, 0)):
        refused(L.isi_vq_finalize_f32(ok, n_part, ok, K, N, D, ok, None), b"vq_finalize: bad argument")
    refused(L.isi_vq_finalize_f32(ok, 1, None, 8, 8, 8, ok, None), b"vq_finalize: bad argument")
    refused(L.isi_vq_ema_update_f32(ok, ok, ok, ok, ok, 0, 8, 0.99, 1e-5, None), b"vq_ema_update: bad argument")
    refused(L.isi_vq_ema_update_f32(ok, ok, ok, ok, ok, 8, 0, 0.99, 1e-5, None), b"vq_ema_update: bad argument")
    for i in range(5):
        p = [ok] * 5
        p[i] = None
        refused(L.isi_vq_ema_update_f32(*p, 8, 8, 0.99, 1e-5, None), b"vq_ema_update: bad argument")
    # embed_code: D % 4, and (new) alignment of the float4 operands (the int64 indices are read as scalars)
    for N, D, K in ((0, 8, 8), (3, 6, 8), (3, 0, 8), (3, 8, 0)):
        refused(L.isi_embed_code_f32(ok, ok, ok, N, D, K, None), b"embed_code: bad argument")
    refused(L.isi_embed_code_f32(ok, odd, ok, 3, 8, 8, None), b"embed_code: codes and out must be 16-byte aligned")
    refused(L.isi_embed_code_f32(ok, ok, odd, 3, 8, 8, None), b"embed_code: codes and out must be 16-byte aligned")
    # pair format, relu_inplace, pad_channels4
    for fn, name in ((L.isi_pair_encode_f32, b"pair_encode"), (L.isi_pair_decode_f32, b"pair_decode")):
        refused(fn(ok, ok, 12, None), name + b": need a multiple of 8 elements")
        refused(fn(odd, ok, 8, None), name + b": pointers must be 16-byte aligned")
        refused(fn(ok, odd, 8, None), name + b": pointers must be 16-byte aligned")
        assert fn(ok, ok, 0, None) == 0
    refused(L.isi_relu_inplace_f32(None, 8, None), b"relu_inplace: bad argument")
    refused(L.isi_relu_inplace_f32(ok, -1, None), b"relu_inplace: bad argument")
    assert L.isi_relu_inplace_f32(ok, 0, None) == 0
    src = _hip.isi_src(ok, 2, 2 * 1025 * 2048, 1025 * 2048, 2048, 1)
    refused(L.isi_pad_channels4_f32(C.byref(src), odd, 1, 1025, 2048, None), b"pad_channels4: output must be 16-byte aligned")


def test_path_choosing_helpers_at_the_edges_of_the_gpu_cases():
    from interactive_spectrogram_inpainting import _hip
    L = _hip.lib()
    for M, want in ((1, 1), (3, 1), (4, 1), (255, 1), (256, 1), (257, 2), (65536, 256), (65537, 256), (70001, 256)):
        assert L.isi_colsum_num_partials(M) == want, M
    for n, want in ((1, 1), (3, 1), (4, 1), (5, 1), (1027, 1), (1028, 2), (4 * 1024 * 256, 1024), (4 * 1024 * 256 + 1203, 1024),
                    (4 * CAP + 1203, 1024)):
        assert L.isi_mse_loss_num_partials(n) == want, n
    # the route of colsum_f32 as the GPU cases name it
    assert TS.colsum_route(256, 64, 64, 0x10000) == "flat" and TS.colsum_route(4, 1, 1, 0x10000) == "flat"
    assert TS.colsum_route(256, 64, 128, 0x10000) == "partial"              # strided
    assert TS.colsum_route(256, 64, 64, 0x10004) == "partial"               # dense, off by 4 bytes
    assert TS.colsum_route(3, 1, 1, 0x10000) == "partial"                   # M C % 4
    assert TS.colsum_route(4, 3, 3, 0x10000) == "partial" and TS.colsum_route(4, 2048, 2048, 0x10000) == "partial"
    assert TS.colsum_route(1, 1024, 1024, 0x10000) == "flat" and TS.colsum_route(4, 1025, 1025, 0x10000) == "partial"
