"""WorldPipeline facade, synthetic map source, persistence and wire formats on the GPU (SURVEY.md 8b face 2, 8f-2/3/4)."""
import numpy as np
import pytest
import torch

from conftest import rel_rms
from _engine_opts import engine_options_guard, pinned  # noqa: F401  (the guard is an autouse fixture: every test here starts and ends on the shipped options)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def td():
    import terrain_diffusion_amd as t
    assert torch.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def models(td):
    from oracle.unet import COARSE_CONFIG, DECODER_CONFIG, synth_state_dict, tiny_config
    bcfg = tiny_config(64, 1)
    ms = [td.EDMUnet2D(**c, dtype="fp32").load_state_dict(synth_state_dict(c, seed=s)) for c, s in ((COARSE_CONFIG, 1), (bcfg, 2), (DECODER_CONFIG, 3))]
    yield ms
    for m in ms:
        m.close()


def _world(td, models, **kw):
    return td.WorldPipeline.from_models(*models, seed=4242, decoder_tile_size=64, decoder_tile_stride=48, latents_batch_size=16, **kw).bind()


def test_perlin_map_kernel_vs_numpy_twin(td):
    from oracle import synthmap
    from terrain_diffusion_amd.engine import get_engine
    from terrain_diffusion_amd.synthetic_map import make_synthetic_map_factory
    f = make_synthetic_map_factory(get_engine("cuda"), frequency_mult=[1.5, 3, 3, 3, 3], seed=77)
    for ch in (0, 1, 4):
        fr, o, l, g = f.params[ch]
        src, dst = f.stats["noise_quantile_tables"][ch].astype(np.float32), f.stats["data_quantile_tables"][ch].astype(np.float32)
        got = f._channel(ch, -37, 1200, 50, 70).cpu().numpy()
        ref = synthmap.fbm_map(50, 70, -37, 1200, f.seeds[ch], fr, o, l, g, src, dst)
        scale = np.abs(dst).max()
        assert np.abs(got - ref).max() < 2e-4 * scale, ch      # fast sin/cos intrinsics on the device: ~1e-6 in the noise, stretched by the transfer
    raw = f.sample_raw(10, 20, 42, 84)
    fin = f.finalize(raw).cpu().numpy()
    s = f.stats
    assert np.allclose(fin, synthmap.finalize(raw.cpu().numpy(), s["a_temp_std"], s["b_temp_std"], s["temp_std_p1"], s["temp_std_p99"]), rtol=1e-5, atol=1e-3)
    full = f(10, 20, 42, 84)
    assert full.shape == (5, 32, 64) and torch.isfinite(full).all()
    # the field is a function of absolute coordinates: overlapping (square) requests agree
    assert torch.equal(f.sample_raw(0, 0, 16, 16)[:, 4:, 4:], f.sample_raw(4, 4, 16, 16))
    # reference orientation (synthetic_map.py:207-218, np.meshgrid(x, y) in 'xy' order): a square request is the TRANSPOSE of the kernel's natural order
    assert torch.equal(f.sample_raw(-5, 9, 19, 33)[2], f._channel(2, -5, 9, 24, 24).t())


def test_conditioning_windows_agree_on_shared_cells(td, models):
    """The coarse stage asks for its conditioning window by window (world_pipeline.py:884-907, with the reference's (i, j) -> (j, i) swap):
    two overlapping windows must see the same value at the same world cell, whatever their origins (round-2 advisor finding: the factory used
    the natural orientation, so the swap made the value depend on the window origin and coarse tiles were blended from unrelated maps)."""
    w = _world(td, models)
    a = w._conditioning_model_input(0, 64, 0, 64)           # rows [0, 64) x cols [0, 64)
    b = w._conditioning_model_input(48, 112, 0, 64)          # next window down: shares rows [48, 64)
    c = w._conditioning_model_input(16, 80, -32, 32)         # diagonal neighbour: shares rows [16, 64) x cols [0, 32)
    assert torch.equal(a[:, 48:, :], b[:, :16, :])
    assert torch.equal(a[:, 16:, :32], c[:, :48, 32:])
    # a custom import is placed in world orientation and merged with the same field (no `finalize`, world_pipeline.py:862-880)
    imp = np.full((8, 8), 123.0, np.float32)
    w.set_custom_conditioning_import(1, imp, 52, 4)
    a2, b2 = w._conditioning_model_input(0, 64, 0, 64), w._conditioning_model_input(48, 112, 0, 64)
    assert torch.equal(a2[:, 48:, :], b2[:, :16, :])
    assert bool((a2[1, 52:60, 4:12] == 123.0).all()) and bool((b2[1, 4:12, 4:12] == 123.0).all())
    w.close()


def test_world_pipeline_get_matches_oracle_composition(td, models):
    """get() = _compute_elev + _compute_climate over the pipeline's own stage tensors: compared with the CPU oracle's composition of host
    copies of those tensors (oracle/compose.py), for a box that is not aligned to anything; deterministic; seed-dependent."""
    from oracle import compose
    w = _world(td, models)
    box = (-21, 13, 75, 141)
    out = w.get(*box)
    elev, clim = out["elev"], out["climate"]
    assert elev.is_cuda and elev.shape == (96, 128) and clim.shape == (5, 96, 128) and torch.isfinite(elev).all() and torch.isfinite(clim).all()

    class Host:
        def __init__(self, t):
            self.t = t

        def __getitem__(self, idx):
            return torch.as_tensor(self.t[idx]).cpu()
    ref_e = compose.compute_elev(Host(w.residual), Host(w.latents), *box, 8, w.kwargs["residual_mean"], w.kwargs["residual_std"])
    ref_c = compose.compute_climate(Host(w.coarse), *box, ref_e, 8)
    assert rel_rms(elev.cpu().numpy(), ref_e.numpy()) < 1e-5 and rel_rms(clim.cpu().numpy(), ref_c.numpy()) < 1e-5
    again = w.get(*box)
    assert torch.equal(again["elev"], elev) and torch.equal(again["climate"], clim)
    n0 = w.residual.windows_computed
    w.empty_cache()
    with pinned(w.engine, batch_invariant=1):
        a = w.get(*box)["elev"]
        w.get(-200, -180, -150, -100, with_climate=False)   # another region first: the windows of `box` are then recomputed in other batches
        w.empty_cache()
        w.get(-21, 13, 27, 77, with_climate=False)          # (a sub-box is NOT the crop of the box: the Laplacian re-encode sees another extent,
        b = w.get(*box)["elev"]                             #  as in the reference; the same box after a flush must give the same bits)
        assert torch.equal(b, a)
    assert w.residual.windows_computed > n0
    assert w.change_seed(4243) and not w.change_seed(4243)
    assert not torch.equal(w.get(*box, with_climate=False)["elev"], elev)
    w.close()


def test_world_pipeline_persistent_store_and_wire_format(td, models, tmp_path):
    from terrain_diffusion_amd import wire
    path = str(tmp_path / "world")
    w = _world_indirect(td, models, path)
    box = (0, 0, 64, 96)
    out = w.get(*box)
    assert w.tile_store.params["seed"] == 4242
    payload, hdr = wire.binary_payload(out["elev"], out["climate"])
    assert len(payload) == 64 * 96 * 2 + 64 * 96 * 16 and hdr == {"X-Height": "64", "X-Width": "96"}
    e16, c4 = wire.parse_payload(payload, 64, 96)
    assert np.array_equal(e16, np.clip(np.floor(out["elev"].cpu().numpy()), -32768, 32767).astype(np.int16))
    assert np.array_equal(c4, out["climate"][:4].cpu().numpy())
    w.close()
    # reopen: every window comes from disk, nothing is recomputed, bytes identical
    calls = []
    w2 = _world_indirect(td, models, path)
    f0 = w2.residual.f
    w2.residual.f = lambda *a, **k: (calls.append(1), f0(*a, **k))[1]
    out2 = w2.get(*box)
    assert not calls and torch.equal(out2["elev"], out["elev"]) and torch.equal(out2["climate"], out["climate"])
    w2.close()


def test_world_file_parameter_mismatch_policy_and_temp_world(td, models, tmp_path):
    """world_pipeline.py:625-664: a world file records seed + kwargs.  Reopened with another seed the reference asks on the console; here
    on_param_mismatch decides and the default ('stored', the reference's default answer) is LOUD (round-2 review: it was silent)."""
    import os
    path = str(tmp_path / "world2")
    mk = lambda seed: td.WorldPipeline.from_models(*models, seed=seed, decoder_tile_size=64, decoder_tile_stride=48, latents_batch_size=16, caching_strategy="indirect")
    w = mk(4242).bind(path); w.close()
    with pytest.warns(UserWarning, match="other parameters"):
        w = mk(7).bind(path)
    assert w.seed == 4242 and w.tile_store.params["seed"] == 4242
    w.close()
    with pytest.raises(ValueError, match="other parameters"):
        mk(7).bind(path, on_param_mismatch="error")
    w = mk(7).bind(path, on_param_mismatch="overwrite")
    assert w.seed == 7 and w.tile_store.params["seed"] == 7
    w.close()
    # 'TEMP' (world_pipeline.py:28-36, 711-713): a temporary world that close() removes
    w = mk(11).bind("TEMP")
    tmp = w._temp_dir
    assert os.path.isdir(tmp) and w.tile_store.params["seed"] == 11
    w.close()
    assert not os.path.exists(tmp)


def test_device_window_tensor_integer_indices_drop_their_dimension(td, models):
    """Round-2 advisor: in the channel-subset branch only dim 0 was squeezed (t[0, 5, :] kept a size-1 dimension)."""
    w = _world(td, models)
    t = w.coarse
    full = t[:, 3:9, 2:12]
    assert t[0, 5, 2:12].shape == (10,) and torch.equal(t[0, 5, 2:12], full[0, 2])
    assert t[1:3, 4, 2:12].shape == (2, 10) and torch.equal(t[1:3, 4, 2:12], full[1:3, 1])
    assert t[:, 4, 7].shape == (full.shape[0],) and torch.equal(t[:, 4, 7], full[:, 1, 5])
    w.close()


def test_large_region_read_is_cut_along_the_window_grid_bit_identically(td, models):
    """Round-4 advisor: a single large region went through the region-gather kernel with EVERY window it touches listed per pixel.  Large regions are
    now cut into cells of <= MAX_REGION_WINDOWS windows (DeviceWindowTensor._gather_cells); same windows, same order: the same bits."""
    w = _world(td, models)
    t = w.latents
    y0, x0, h, wd = -37, 11, 300, 333            # straddles the origin, not aligned to the window grid, dozens of windows
    assert len(t._windows_for([0, y0, x0], [t.channels + 1, y0 + h, x0 + wd])) > t.MAX_REGION_WINDOWS
    cut = t[:, y0:y0 + h, x0:x0 + wd]
    keep, type(t).MAX_REGION_WINDOWS = t.MAX_REGION_WINDOWS, 1 << 30
    try:
        whole = t[:, y0:y0 + h, x0:x0 + wd]      # the one-region path
    finally:
        type(t).MAX_REGION_WINDOWS = keep
    assert cut.shape == whole.shape == (t.channels + 1, h, wd) and torch.equal(cut, whole)
    sub = t[:, y0 + 50:y0 + 90, x0 + 60:x0 + 100]   # a small region (one-region path) agrees with the crop of the large one
    assert torch.equal(sub, cut[:, 50:90, 60:100])
    # Round-5 advisor: with a window store smaller than the region (the cascade bench's default cache is 100 MiB) the early windows used to be evicted
    # before their cell's gather ran and were evaluated again.  The read now holds the windows it ensured: every window of the region once, same bits.
    n_win = len(t._windows_for([0, y0, x0], [t.channels + 1, y0 + h, x0 + wd]))
    t.tile_store.clear(t.tensor_id)
    keep_bytes, t.tile_store.cache_size_bytes = t.tile_store.cache_size_bytes, 4 * t.channels * t.tile * t.tile * 4   # room for four windows
    try:
        n0 = t.windows_computed
        again = t[:, y0:y0 + h, x0:x0 + wd]
        assert t.windows_computed - n0 == n_win, (t.windows_computed - n0, n_win)
    finally:
        t.tile_store.cache_size_bytes = keep_bytes
    # (the store is shared with the upstream tensors: their evicted windows are recomputed in other batch compositions, which in the default -- not
    # batch-invariant -- plan may round differently; the count above is the point, the values only have to agree to bf16 accuracy)
    assert rel_rms(again.cpu().numpy(), cut.cpu().numpy()) < 2e-2
    w.close()


def test_world_pipeline_to_is_loud(td, models):
    """Round-2 review: `to()` silently ignored its argument.  The resident device is accepted, everything else is refused."""
    w = _world(td, models)
    assert w.to("cuda") is w and w.to(torch.device("cuda", 0)) is w and w.to(0) is w
    with pytest.raises(RuntimeError):
        w.to("cpu")
    with pytest.raises(RuntimeError):
        w.to("cuda:5")
    with pytest.raises(TypeError):
        w.to(torch.float16)
    w.close()


def test_measure_latency_harness_on_a_given_world(td, models):
    """evaluation/latency.py:19-127 twin: drives to() / bind('TEMP') / get(with_climate=False) / empty_cache() / close() the way the reference's
    harness does and returns its result keys; the second tile must not be slower than a cold one on average over a few runs."""
    from terrain_diffusion_amd.latency import measure_latency
    w = td.WorldPipeline.from_models(*models, seed=77, decoder_tile_size=64, decoder_tile_stride=48, latents_batch_size=[1, 2, 4, 8, 16], cache_limit=None)
    r = measure_latency(world=w, num_runs=3, tile_size=128)
    for k in ("ttft_mean", "ttst_mean", "ttft_std", "ttst_std", "ttft_p5", "ttft_p50", "ttft_p95", "ttst_p5", "ttst_p50", "ttst_p95", "peak_vram_mb"):
        assert k in r and r[k] >= 0.0, k
    assert 0.0 < r["ttst_mean"] <= r["ttft_mean"] * 1.5, r


def _world_indirect(td, models, path):
    return td.WorldPipeline.from_models(*models, seed=4242, decoder_tile_size=64, decoder_tile_stride=48, latents_batch_size=16,
                                        caching_strategy="indirect").bind(path)


def test_save_pretrained_round_trip(td, models, tmp_path):
    """save_pretrained writes the reference's layout (world_pipeline.py:500-518: config.json + coarse_model/ base_model/ decoder_model/, each a
    config.json + one safetensors state dict under the reference's parameter names); from_pretrained on that directory rebuilds a pipeline
    that serves the same bytes."""
    import json
    import os
    from safetensors.torch import load_file
    w = _world(td, models)
    box = (5, -9, 69, 71)
    ref = w.get(*box)
    root = str(tmp_path / "pipe")
    w.save_pretrained(root)
    assert sorted(os.listdir(root)) == ["base_model", "coarse_model", "config.json", "decoder_model"]
    cfg = json.load(open(os.path.join(root, "config.json")))
    assert cfg["_class_name"] == "WorldPipeline" and cfg["decoder_tile_size"] == 64 and "seed" not in cfg
    sd = load_file(os.path.join(root, "base_model", "diffusion_pytorch_model.safetensors"))
    assert set(models[1].expected_parameters()) <= set(sd) and all(v.dtype == torch.float32 for v in sd.values())
    w2 = td.WorldPipeline.from_pretrained(root, seed=4242, latents_batch_size=16, dtype=None).bind()
    got = w2.get(*box)
    assert torch.equal(got["elev"], ref["elev"]) and torch.equal(got["climate"], ref["climate"])
    w2.close()
    for m in (w2.coarse_model, w2.base_model, w2.decoder_model):
        m.close()
    w.close()


def test_request_replica_mode_two_ranks_serve_the_same_world(td, models):
    """BASELINE configs[4] on several GPUs: every rank holds the whole lazy graph of ONE world (same seed) and serves a
    spatially compact share of the request boxes (parallel.shard_requests); no window crosses a GPU boundary.  Two 'ranks' (two pipelines on this
    GPU) must return exactly what one pipeline returns for the same boxes -- bit for bit in batch-invariant mode, where a window's value does
    not depend on the batch it was computed in."""
    from terrain_diffusion_amd.engine import get_engine
    from terrain_diffusion_amd.parallel import shard_requests
    eng = get_engine("cuda")
    with pinned(eng, batch_invariant=1):
        boxes = [(64 * a - 40, 64 * b + 8, 64 * a + 24, 64 * b + 72) for a in range(3) for b in range(2)]
        one = _world(td, models)
        ref = [one.get(*bx, with_climate=False)["elev"].clone() for bx in boxes]
        one.close()
        got = {}
        for r in range(2):
            w = _world(td, models)
            for k, bx in shard_requests(boxes, world=2, rank=r):
                got[k] = w.get(*bx, with_climate=False)["elev"].clone()
            w.close()
        assert sorted(got) == list(range(len(boxes)))
        for k in range(len(boxes)):
            assert torch.equal(got[k], ref[k]), k


def test_enqueue_only_cascade_gives_the_bits_of_the_synchronous_one(td, models):
    """Engine.on_stream (td_engine_set_stream + option "async"): every stage of the cascade -- noise, samplers, region gathers, resampling,
    elevation / climate composition -- only ENQUEUES on the stream it shares with torch (host arrays go through the engine's pinned ring, scratch
    through its stream-ordered pool) instead of completing on return.  Same world, same requests, same bits; and the window cache is small enough
    that windows are evicted and released while work that reads them may still be queued."""
    from terrain_diffusion_amd.engine import get_engine
    eng = get_engine("cuda")
    boxes = [(-40, 30, 150, 190), (90, 100, 260, 300), (-40, 30, 150, 190), (1000, -900, 1130, -720)]
    # ... and enough further requests that the engine's pinned staging ring (2 x 2 MiB of descriptor / tap tables) wraps at least once
    boxes += [(5000 + 173 * k, -3000 + 131 * (k % 7), 5000 + 173 * k + 140, -3000 + 131 * (k % 7) + 150) for k in range(44)]
    ref_w = _world(td, models, cache_limit=2 * 2 ** 20)
    ref = [ref_w.get(*b) for b in boxes]
    ref_w.close()
    w = _world(td, models, cache_limit=2 * 2 ** 20)
    with eng.on_stream(torch.cuda.Stream()):
        got = [w.get(*b) for b in boxes]        # nothing in here waits for the GPU
        eng.synchronize()
    torch.cuda.synchronize()
    for b, r, g in zip(boxes, ref, got):
        assert torch.equal(r["elev"], g["elev"]), b
        assert torch.equal(r["climate"], g["climate"]), b
    assert w.tile_store.evictions > 0
    w.close()
