"""Host-side checks of the EMA codebook with random restarts (vqvae/bottleneck.py: QuantizedBottleneckWithRestarts): the
model builds it, the row hash the kernels call is pinned to the written specification (tests/restarts_spec.py) through
its host export, a plain bottleneck's checkpoint loads without re-initialising the codebook, and the candidate table rides
in the EMA-statistics message.  No GPU needed."""
import socket
import warnings

import numpy as np
import pytest
import torch

import restarts_spec as S


def test_vqvae_builds_the_bottleneck_with_restarts_and_keeps_the_plain_one_at_threshold_one(tmp_path):
    from interactive_spectrogram_inpainting.vqvae.bottleneck import QuantizedBottleneck, QuantizedBottleneckWithRestarts
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    m = VQVAE(in_channel=2, restarts_usage_threshold=0.5)
    for q in (m.quantize_t, m.quantize_b):
        assert type(q) is QuantizedBottleneckWithRestarts and isinstance(q, QuantizedBottleneck)
        assert q.restart_threshold == 0.5 and q.corruption_weights is None and q.initialize
        assert q.restart_state.dtype == torch.int64 and q.restart_state.tolist() == [0, 0, 0, 0]
    sd = m.state_dict()
    assert "quantize_t.restart_state" in sd and "quantize_b.restart_state" in sd
    path = tmp_path / "model.json"
    m.store_instantiation_parameters(str(path))
    torch.save(sd, tmp_path / "weights.pt")
    m2 = VQVAE.from_parameters_and_weights(path, tmp_path / "weights.pt")
    assert m2.restarts_usage_threshold == 0.5
    assert type(m2.quantize_t) is QuantizedBottleneckWithRestarts and type(m2.quantize_b) is QuantizedBottleneckWithRestarts
    assert set(m2.state_dict()) == set(sd)
    plain = VQVAE(in_channel=2, restarts_usage_threshold=1.)
    assert type(plain.quantize_t) is QuantizedBottleneck and type(plain.quantize_b) is QuantizedBottleneck
    assert set(plain.state_dict()) == set(sd) - {"quantize_t.restart_state", "quantize_b.restart_state"}
    assert set(plain.state_dict()) == set(VQVAE(in_channel=2).state_dict())
    off = VQVAE(in_channel=2, restarts_usage_threshold=0.5, disable_quantization=True)
    assert type(off.quantize_t).__name__ == "UnquantizedBottleneck"


def test_spec_mix_is_splitmix64s_finaliser():
    """The published first output of splitmix64 seeded with 0: mix(0 + golden gamma)."""
    assert S.mix(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    assert S.mix(0) == 0


def test_exported_row_hash_equals_the_spec():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    assert "isi_vq_restart_row" in _hip.SIGNATURES
    for name in ("isi_vq_restart_candidates_f32", "isi_vq_ema_update_restart_f32"):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    known = {(0, 0, 0, 4096): 0, (1, 1, 511, 37): 24, (1 << 63, 1 << 32, 2047, 262144): 157095,
             ((1 << 64) - 1, (1 << 40) + 3, 1, 2): 0, (0, 1, 0, 262144): 40164, (1, 0, 511, 4096): 999, (7, 5, 3, 1): 0}
    for args, want in known.items():
        assert S.row(*args) == want, args
        assert lib.isi_vq_restart_row(*args) == want, args
    seen = set()
    for seed in (0, 1, 1 << 63, (1 << 64) - 1):
        for step in (0, 1, 1 << 32, (1 << 40) + 3):
            for k in (0, 1, 511, 2047):
                for N in (1, 2, 37, 4096, 262144):
                    got = lib.isi_vq_restart_row(seed, step, k, N)
                    assert got == S.row(seed, step, k, N), (seed, step, k, N)
                    assert 0 <= got < N
                    if N == 262144:
                        seen.add(got)
    assert len(seen) > 50, "the 64 draws at N = 262144 must not collapse onto a few rows"


def test_argument_checks_run_before_any_launch():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    fake = 0x10000
    assert lib.isi_vq_restart_candidates_f32(None, 4, 8, 5, fake, 0, 1, fake, None) == -1
    assert lib.isi_vq_restart_candidates_f32(fake, 0, 8, 5, fake, 0, 1, fake, None) == -1
    assert lib.isi_vq_restart_candidates_f32(fake, 4, 8, 5, fake, 2, 2, fake, None) == -1      # rank outside the world
    assert lib.isi_vq_restart_candidates_f32(fake, 4, 8, 5, None, 0, 1, fake, None) == -1
    ok = [fake] * 6
    assert lib.isi_vq_ema_update_restart_f32(*ok, 8, 5, 0.99, 1e-5, 0.5, 1, None, None) == -1
    assert lib.isi_vq_ema_update_restart_f32(*ok[:5], None, 8, 5, 0.99, 1e-5, 0.5, 1, fake, None) == -1
    assert lib.isi_vq_ema_update_restart_f32(*ok, 8, 65537, 0.99, 1e-5, 0.5, 1, fake, None) == -1


def test_plain_checkpoint_loads_with_step_one_and_a_warning():
    from interactive_spectrogram_inpainting.vqvae.bottleneck import QuantizedBottleneck, QuantizedBottleneckWithRestarts
    torch.manual_seed(3)
    plain = QuantizedBottleneck(8, 16)
    plain.cluster_size.uniform_(0, 4)
    q = QuantizedBottleneckWithRestarts(8, 16, restart_threshold=0.5, seed=(1 << 64) - 3)
    assert q.restart_state.tolist() == [-3, 0, 0, 0]       # the seed's 64 bits in the int64 buffer
    with pytest.warns(UserWarning, match="restart_state"):
        q.load_state_dict(plain.state_dict())
    assert q.restart_state.tolist() == [-3, 1, 0, 0]
    for name in ("embed", "cluster_size", "embed_avg"):
        assert torch.equal(getattr(q, name), getattr(plain, name))
    # its own checkpoint round-trips silently, step included
    q.restart_state.copy_(torch.tensor([11, 7, 2, 9]))
    q2 = QuantizedBottleneckWithRestarts(8, 16, restart_threshold=0.5)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        q2.load_state_dict(q.state_dict())
    assert q2.restart_state.tolist() == [11, 7, 2, 9]
    # and the whole model: a plain model's checkpoint into a model with restarts
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    m = VQVAE(in_channel=2, restarts_usage_threshold=0.5)
    with pytest.warns(UserWarning, match="restart_state"):
        m.load_state_dict(VQVAE(in_channel=2).state_dict())
    assert m.quantize_t.restart_state.tolist() == [0, 1, 0, 0] and m.quantize_b.restart_state.tolist() == [0, 1, 0, 0]


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


_D, _K, _N, _SEED, _STEP = 8, 16, 40, 12345, 3


def _restart_worker(rank, world, port, q):
    import os
    import pathlib
    import sys
    root = pathlib.Path(__file__).resolve().parent.parent
    for p in (root / "interactive-spectrogram-inpainting_amd", root, root / "tests"):
        sys.path.insert(0, str(p))
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from interactive_spectrogram_inpainting.vqvae._train import exchange_ema_statistics
    import restarts_spec as spec
    g = torch.Generator().manual_seed(5)
    z = torch.randn(_N, _D, generator=g)
    mine = z[rank::world].numpy()
    cand, bad = spec.candidates(mine, _SEED, _STEP, _K, rank, world)
    assert not cand[(rank + 1) % world::world].any()       # zero outside this rank's codes
    table = torch.from_numpy(np.concatenate([cand.reshape(-1), bad]))
    counts = torch.full((_K,), float(rank + 1))
    embed_sum = torch.full((_D, _K), float(10 * (rank + 1)))
    counts, embed_sum, table = exchange_ema_statistics(counts, embed_sum, table)
    two = exchange_ema_statistics(torch.ones(_K), torch.ones(_D, _K))      # the two-part form still returns two parts
    q.put((rank, counts.tolist(), embed_sum.tolist(), table.tolist(), len(two)))
    dist.barrier()
    dist.destroy_process_group()


def test_candidates_travel_in_the_ema_statistics_message_gloo():
    """World of 2: each rank passes the candidates of its own codes (zero elsewhere); after the one all-reduce both hold
    the full table -- row(seed, step, k, N_r) of shard k mod 2 -- next to the summed counts and sums."""
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_restart_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    g = torch.Generator().manual_seed(5)
    z = torch.randn(_N, _D, generator=g).numpy()
    want = np.zeros((_K, _D), dtype=np.float32)
    for k in range(_K):
        shard = z[k % world::world]
        want[k] = shard[S.row(_SEED, _STEP, k, shard.shape[0])]
    assert sorted(o[0] for o in out) == [0, 1]
    for rank, counts, embed_sum, table, n_two in out:
        table = np.asarray(table, dtype=np.float32)
        assert np.array_equal(table[:_K * _D].reshape(_K, _D), want)
        assert not table[_K * _D:].any()
        assert counts == [3.0] * _K and np.all(np.asarray(embed_sum) == 30.0)
        assert n_two == 2


def test_exchange_without_a_process_group_is_the_identity():
    from interactive_spectrogram_inpainting.vqvae._train import exchange_ema_statistics
    a, b, c = torch.ones(4), torch.ones(2, 4), torch.ones(12)
    out = exchange_ema_statistics(a, b, c)
    assert len(out) == 3 and out[0] is a and out[1] is b and out[2] is c
    assert len(exchange_ema_statistics(a, b)) == 2
