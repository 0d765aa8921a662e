"""The EMA codebook with random restarts of dead codes on the GPU: the candidate gather and the update kernel against the
written specification (tests/restarts_spec.py), the bottleneck module against the plain one, and the training step of a
model with restarts eager, replayed from a HIP graph, and with the fused / unfused quantiser launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import restarts_spec as S

pytestmark = pytest.mark.gpu

_SEED = (1 << 63) + 5            # exercises the top bit of the int64 buffer
_STEP = (1 << 32) + 7


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _i64(v: int) -> int:
    return v - (1 << 64) if v >= (1 << 63) else v


def _state(seed, step, last=0, total=0):
    return torch.tensor([_i64(seed), step, last, total], dtype=torch.int64, device=_dev())


def _candidates(z, K, state, rank=0, world=1, out=None):
    from interactive_spectrogram_inpainting import _hip
    N, D = z.shape
    if out is None:
        out = torch.full((K * D + K,), -7.0, device=z.device)      # every word must be written
    _hip.check(_hip.lib().isi_vq_restart_candidates_f32(z.data_ptr(), N, D, K, state.data_ptr(), rank, world, out.data_ptr(),
                                                        C.c_void_p(_hip.stream_ptr(z.device))), "isi_vq_restart_candidates_f32")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o[:K * D].reshape(K, D), o[K * D:]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2), (2, 3)])
@pytest.mark.parametrize("N,D,K", [(1, 8, 5), (37, 64, 5), (4096, 64, 512), (100, 6, 33)])
def test_candidates_kernel_equals_the_spec_bitwise(N, D, K, rank, world):
    """(100, 6, 33): the scalar path (D % 4 != 0); the others read and write float4."""
    z = torch.randn(N, D, generator=torch.Generator().manual_seed(N + D + K))
    cand, bad = _candidates(z.to(_dev()), K, _state(_SEED, _STEP), rank, world)
    want, want_bad = S.candidates(z.numpy(), _SEED, _STEP, K, rank, world)
    assert np.array_equal(_bits(cand), _bits(want))
    assert np.array_equal(bad, want_bad) and not bad.any()
    if world > 1:
        assert want[rank::world].any() and not want[(rank + 1) % world::world].any()


def test_candidates_written_inside_a_packed_message_take_the_scalar_path():
    """K = 5, D = 8: the table starts K + D K = 45 floats into the statistics message -- not 16-byte aligned."""
    N, D, K = 37, 8, 5
    z = torch.randn(N, D, generator=torch.Generator().manual_seed(2))
    msg = torch.zeros(K + D * K + K * D + K, device=_dev())
    out = msg[K + D * K:]
    assert out.data_ptr() % 16 != 0
    cand, bad = _candidates(z.to(_dev()), K, _state(3, 9), out=out)
    want, _ = S.candidates(z.numpy(), 3, 9, K)
    assert np.array_equal(_bits(cand), _bits(want)) and not bad.any()
    assert not msg[:K + D * K].any()


def test_candidates_with_non_finite_rows_are_zeroed_and_flagged():
    N, D, K = 37, 64, 5
    z = torch.randn(N, D, generator=torch.Generator().manual_seed(11))
    r1, r3 = S.row(_SEED, _STEP, 1, N), S.row(_SEED, _STEP, 3, N)
    assert r1 != r3
    z[r1, 7] = float("nan")
    z[r3, 63] = float("-inf")
    cand, bad = _candidates(z.to(_dev()), K, _state(_SEED, _STEP))
    want, want_bad = S.candidates(z.numpy(), _SEED, _STEP, K)
    assert want_bad[1] == 1 and want_bad[3] == 1 and not want[1].any() and not want[3].any()
    assert np.array_equal(_bits(cand), _bits(want)) and np.array_equal(bad, want_bad)
    assert np.isfinite(cand).all()


def test_two_ranks_shards_sum_to_the_full_table():
    D, K = 64, 33
    g = torch.Generator().manual_seed(4)
    shards = [torch.randn(37, D, generator=g), torch.randn(50, D, generator=g)]
    state = _state(_SEED, _STEP)
    parts = [_candidates(z.to(_dev()), K, state, r, 2) for r, z in enumerate(shards)]
    total = parts[0][0] + parts[1][0]
    for k in range(K):
        z = shards[k % 2]
        assert np.array_equal(_bits(total[k]), _bits(z[S.row(_SEED, _STEP, k, z.shape[0])].numpy())), k
    assert not (parts[0][1] + parts[1][1]).any()


# ------------------------------------------------------------------ update kernel
def _inputs(D, K, seed, dead=(), flagged=()):
    """Buffers and statistics without cancellation in embed_avg's update (the sums share embed_avg's signs, as sums of the
    vectors a code attracts do), so that an element-wise relative bound is meaningful.  `dead`: cluster sizes far below
    0.5 and no vectors this step; `flagged`: dead ones whose candidate is flagged."""
    rng = np.random.default_rng(seed)
    embed = rng.standard_normal((D, K)).astype(np.float32)
    cs = rng.uniform(2.0, 6.0, K).astype(np.float32)
    counts = rng.integers(0, 11, K).astype(np.float32)
    dead = np.asarray(sorted(dead), dtype=np.int64)
    cs[dead] = rng.uniform(0.01, 0.2, dead.size).astype(np.float32)
    counts[dead] = 0
    ea = (embed * cs[None, :]).astype(np.float32)
    esum = (np.sign(ea) * np.abs(rng.standard_normal((D, K))) * counts[None, :]).astype(np.float32)
    cand = rng.standard_normal((K, D)).astype(np.float32)
    bad = np.zeros(K, dtype=np.float32)
    for k in flagged:
        bad[k], cand[k] = 1.0, 0.0
    return embed, cs, ea, counts, esum, cand, bad


def _run_update(embed, cs, ea, counts, esum, cand, bad, state, decay, eps, threshold, initialize, plain=False):
    from interactive_spectrogram_inpainting import _hip
    dev = _dev()
    L = _hip.lib()
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (embed, cs, ea, counts, esum)]
    table = torch.from_numpy(np.concatenate([cand.reshape(-1), bad])).to(dev)
    D, K = embed.shape
    st = _state(*state)
    s = C.c_void_p(_hip.stream_ptr(dev))
    if plain:
        _hip.check(L.isi_vq_ema_update_f32(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                                           D, K, decay, eps, s), "isi_vq_ema_update_f32")
    else:
        _hip.check(L.isi_vq_ema_update_restart_f32(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                                                   t[4].data_ptr(), table.data_ptr(), D, K, decay, eps, threshold,
                                                   int(initialize), st.data_ptr(), s), "isi_vq_ema_update_restart_f32")
    torch.cuda.synchronize()
    return t[0].cpu().numpy(), t[1].cpu().numpy(), t[2].cpu().numpy(), [v if v >= 0 else v + (1 << 64) for v in st.tolist()]


@pytest.mark.parametrize("D", [8, 64])
@pytest.mark.parametrize("K", [5, 512, 1000])
def test_update_without_restarts_is_the_plain_kernel_bit_for_bit(D, K):
    inp = _inputs(D, K, seed=D + K, dead=range(0, K, 3))
    got = _run_update(*inp, (_SEED, 4, 1, 2), 0.99, 1e-5, 0.0, 0)
    ref = _run_update(*inp, (_SEED, 4, 1, 2), 0.99, 1e-5, 0.0, 0, plain=True)
    for a, b in zip(got[:3], ref[:3]):
        assert np.array_equal(_bits(a), _bits(b))
    assert got[3] == [_SEED, 5, 0, 2]


@pytest.mark.parametrize("D,K", [(8, 37), (64, 512)])
def test_update_restarts_the_dead_codes_and_only_them(D, K):
    """Live codes (and the flagged one): the float64 spec to relative 2 K 2^-24 -- n is a sum of K fp32 terms
    (K 2^-24), the quotient's four roundings and the EMA's two stay inside the second K 2^-24.  Dead codes: bitwise."""
    dead = sorted(set(range(1, K, 4)) | {K - 1})
    flagged = [dead[2]]
    thr = 0.5
    inp = _inputs(D, K, seed=K, dead=dead, flagged=flagged)
    embed, cs, ea, state = _run_update(*inp, (_SEED, 6, 0, 10), 0.99, 1e-5, thr, 1)
    w_embed, w_cs, w_ea, w_dead, w_state = S.update(*inp, (_SEED, 6, 0, 10), 0.99, 1e-5, thr, True)
    really_dead = [k for k in dead if k not in flagged]
    assert np.flatnonzero(w_dead).tolist() == really_dead
    cand = inp[5]
    for k in really_dead:
        assert np.array_equal(_bits(embed[:, k]), _bits(cand[k])), k
        assert cs[k] == np.float32(thr)
        assert np.array_equal(_bits(ea[:, k]), _bits(np.float32(thr) * cand[k])), k
    live = ~w_dead
    assert live[flagged[0]]
    bound = 2 * K * 2.0 ** -24
    for got, want, name in ((embed[:, live], w_embed[:, live], "embed"), (cs[live], w_cs[live], "cluster_size"),
                            (ea[:, live], w_ea[:, live], "embed_avg")):
        err = np.max(np.abs(got.astype(np.float64) - want) / np.abs(want))
        print(f"{name}: max relative error {err:.3e} (bound {bound:.3e})")
        assert err <= bound, name
    assert state == list(w_state) == [_SEED, 7, len(really_dead), 10 + len(really_dead)]


def test_initialize_restarts_every_code_at_step_zero_only():
    D, K = 64, 130
    dead = [3, 77]
    inp = _inputs(D, K, seed=1, dead=dead, flagged=[100])
    embed, cs, ea, state = _run_update(*inp, (9, 0, 0, 0), 0.99, 1e-5, 0.5, 1)
    cand = inp[5]
    redrawn = [k for k in range(K) if k != 100]          # a flagged candidate is never taken, not even at step 0
    assert np.array_equal(_bits(embed[:, redrawn]), _bits(cand[redrawn].T))
    assert np.all(cs[redrawn] == np.float32(0.5))
    assert np.array_equal(_bits(ea[:, redrawn]), _bits((np.float32(0.5) * cand[redrawn]).T))
    assert state == [9, 1, K - 1, K - 1]
    one = _run_update(*inp, (9, 1, 0, 0), 0.99, 1e-5, 0.5, 1)
    off = _run_update(*inp, (9, 1, 0, 0), 0.99, 1e-5, 0.5, 0)
    for a, b in zip(one[:3], off[:3]):
        assert np.array_equal(_bits(a), _bits(b))
    assert one[3] == off[3] == [9, 2, 2, 2]
    assert np.array_equal(_bits(one[0][:, dead]), _bits(cand[dead].T))


# ------------------------------------------------------------------ module
def test_module_forward_equals_the_plain_bottleneck_and_revives_the_far_codes():
    from interactive_spectrogram_inpainting.vqvae.bottleneck import QuantizedBottleneck, QuantizedBottleneckWithRestarts
    dev = _dev()
    D, K, far = 64, 64, 32
    g = torch.Generator().manual_seed(8)
    z = torch.randn(2, 8, 16, D, generator=g)
    embed = torch.randn(D, K, generator=g)
    embed[:, far:] += 100.0                      # half the codes far from the data: never chosen
    cs = torch.ones(K)
    cs[far:] = 0.1                               # ... and below the threshold (embed_avg consistent with both)
    seed = 77
    q = QuantizedBottleneckWithRestarts(D, K, restart_threshold=0.5, initialize=False, seed=seed)
    p = QuantizedBottleneck(D, K)
    for m in (q, p):
        m.embed.copy_(embed)
        m.cluster_size.copy_(cs)
        m.embed_avg.copy_(embed * cs[None, :])
        m.to(dev).train()
    zd = z.to(dev)
    out_q, out_p = q(zd), p(zd)
    torch.cuda.synchronize()
    for a, b in zip(out_q, out_p):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert int(out_q[2].max()) < far
    rows = [S.row(seed, 0, k, z.numel() // D) for k in range(far, K)]
    zr = z.reshape(-1, D)
    new = q.embed.cpu()
    for k, r in zip(range(far, K), rows):
        assert torch.equal(new[:, k], zr[r]), k
    assert q.restart_state.tolist() == [seed, 1, K - far, K - far]
    assert float(p.embed[:, far:].min()) > 50.0          # the plain codebook's far codes stay where they were
    used_q = int(torch.unique(q(zd)[2]).numel())
    used_p = int(torch.unique(p(zd)[2]).numel())
    torch.cuda.synchronize()
    # every distinct restarted row is its own nearest code at distance 0; the near codes that were in use lose at most those rows
    assert used_q >= len(set(rows))
    assert used_p <= far and used_q > used_p


# ------------------------------------------------------------------ model
def test_graphed_training_step_with_restarts_equals_eager():
    from interactive_spectrogram_inpainting.utils.training.graphed_step import GraphedTrainingStep
    from interactive_spectrogram_inpainting.utils.training.optimizer import make_adam
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    dev = _dev()

    def rel(a, b):
        a, b = a.detach().float().cpu(), b.detach().float().cpu()
        return ((a - b).abs().max() / b.abs().max().clamp(min=1e-12)).item()

    def build():
        torch.manual_seed(1)
        m = VQVAE(in_channel=2, restarts_usage_threshold=0.5).to(dev).train()
        return m, make_adam(m.parameters(), lr=1e-3, capturable=True)

    def make_step(m, opt):
        def step(x):
            m.zero_grad()
            out, latent, *_ = m(x)
            loss = torch.nn.functional.mse_loss(out, x) + 0.25 * latent.mean()
            loss.backward()
            opt.step()
            return loss
        return step
    xs = [torch.randn(4, 2, 64, 128, generator=torch.Generator().manual_seed(i)).to(dev) for i in range(4)]
    me, oe = build()
    se = make_step(me, oe)
    le = [float(se(x)) for x in xs]
    mg, og = build()
    g = GraphedTrainingStep(make_step(mg, og), (xs[0].clone(),), warmup=1)
    assert g.n_segments == 1
    lg = [float(g(x)) for x in xs[1:]]
    g.finish()
    for a, b in zip(lg, le[1:]):
        assert abs(a - b) <= 1e-5 * abs(b), (lg, le)
    for (n, pe), pg in zip(me.named_parameters(), mg.parameters()):
        assert rel(pg, pe) < 1e-5, n
    for name in ("quantize_t", "quantize_b"):
        qe, qg = getattr(me, name), getattr(mg, name)
        print(name, "restart_state eager", qe.restart_state.tolist(), "graphed", qg.restart_state.tolist())
        assert torch.equal(qe.restart_state, qg.restart_state)
        st = qe.restart_state.tolist()
        assert st[0] == 0 and st[1] == 4 and st[3] >= qe.n_embed      # four steps; the first redrew every code
        assert rel(qg.embed, qe.embed) < 1e-5


def test_fused_and_unfused_quantiser_launches_restart_the_same_codes():
    from interactive_spectrogram_inpainting.vqvae import _train
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    dev = _dev()
    x = torch.randn(2, 2, 256, 512, generator=torch.Generator().manual_seed(3)).to(dev)
    before, inner = _train.FUSED_QUANTIZER, _train.quantize_conv_train
    got, calls = [], []

    def counted(*a, **kw):
        calls.append(1)
        return inner(*a, **kw)
    try:
        _train.quantize_conv_train = counted
        for fused in (True, False):
            _train.FUSED_QUANTIZER = fused
            torch.manual_seed(1)
            m = VQVAE(in_channel=2, restarts_usage_threshold=0.5).to(dev).train()
            calls.clear()
            with torch.no_grad():
                m(x)
            torch.cuda.synchronize()
            assert len(calls) == (2 if fused else 0), "both quantisers take the fused launch at this shape"
            got.append({k: v.clone() for k, v in m.state_dict().items() if k.startswith("quantize_t.") or k.startswith("quantize_b.")})
    finally:
        _train.FUSED_QUANTIZER, _train.quantize_conv_train = before, inner
    assert got[0]["quantize_t.restart_state"].tolist() == [0, 1, 512, 512]
    for k in got[0]:
        assert torch.equal(got[0][k], got[1][k]), k


def test_train_epoch_reports_restart_totals_eager_and_replayed():
    """`train_vqvae.train` on three batches: `restarts_top` / `restarts_bottom` are the epoch's totals; the replayed epoch
    (GraphedVQVAEStep puts `restart_state` back with the other buffers after its two warm-up steps) ends at step 3 with the
    eager epoch's counts."""
    import train_vqvae as T
    from interactive_spectrogram_inpainting.utils.training.optimizer import make_adam
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    dev = _dev()
    data = T.SyntheticSpectrograms(12, shape=(2, 64, 128))
    res = {}
    for graph in (False, True):
        torch.manual_seed(1)
        m = VQVAE(in_channel=2, restarts_usage_threshold=0.5).to(dev)
        opt = make_adam(m.parameters(), lr=1e-3, capturable=True)
        loader = torch.utils.data.DataLoader(data, batch_size=4, shuffle=False, drop_last=True)
        means = T.train(0, loader, m, torch.nn.MSELoss(), opt, device=dev, hip_graph=graph)
        states = [m.quantize_t.restart_state.tolist(), m.quantize_b.restart_state.tolist()]
        assert states[0][1] == 3 and states[1][1] == 3
        assert means["restarts_top"] == states[0][3] >= 512 and means["restarts_bottom"] == states[1][3] >= 512
        res[graph] = (means, states)
    assert res[True][1] == res[False][1]
    plain = VQVAE(in_channel=2).to(dev)
    means = T.train(0, [(torch.randn(4, 2, 64, 128),)], plain, torch.nn.MSELoss(), make_adam(plain.parameters(), lr=1e-3),
                    device=dev)
    assert set(means) == set(T.RunningMeans.NAMES)
