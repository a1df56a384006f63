"""sha256 of engine outputs on fixed inputs: compares two builds of the library bit for bit.  The base U-Net at batch 64 / 5 / 1 (bf16); an attention-bearing
tiny U-Net (attention in encoder and decoder blocks, with and without a channel change) at 16 x 16, n = 3, and the TINY autoencoder's preencode + decode,
each in fp32 / bf16 / fp16; one 3-step td_sample_edm call, n = 2, on the tiny U-Net (captured graph, fused solver step under the default options); the
entry points that stage host buffers (consistency sampler, noise / blend / normalise, resample, the sampler with guide and score scaling, the grid
batch, the autoencoder's preencode) on tiny shapes, and the profile labels with their launch counts of one sampler call and one autoencoder round trip.
TD_OPTS=key=value,... sets engine options first."""
import sys, os, hashlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(1, os.path.join(sys.path[0], "tests"))
import torch
import terrain_diffusion_amd as td
from terrain_diffusion_amd._lib import lib, check
from terrain_diffusion_amd.engine import ptr
from oracle.unet import BASE_CONFIG, synth_state_dict, tiny_config
from oracle import rng, schedule
import _ae_twin
for kv in os.environ.get("TD_OPTS", "").split(","):
    if kv:
        k, v = kv.split("="); td.engine.get_engine("cuda").set_option(k, int(v))


def sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.float().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


cfg = dict(BASE_CONFIG)
m = td.EDMUnet2D(**cfg, dtype="bf16").load_state_dict(synth_state_dict(cfg, seed=1234))
hs = []
for n in (64, 5, 1):
    x = torch.from_numpy(rng.standard_normal(7, (n, 5, 64, 64))).cuda()
    c = torch.from_numpy(rng.standard_normal(8, (n, 58))).cuda()
    hs.append(sha(m(x, torch.full((n,), 1.1), [c])))
m.close()
lib().td_build_id.restype = __import__("ctypes").c_char_p
print("build", lib().td_build_id().decode(), "output hashes", hs)

cfg = tiny_config(64, 2, image_size=32)
sd = synth_state_dict(cfg, seed=4321)
x = torch.from_numpy(rng.standard_normal(9, (3, 5, 16, 16))).cuda()
c = torch.from_numpy(rng.standard_normal(10, (3, 58))).cuda()
hs = []
for dt in ("fp32", "bf16", "fp16"):
    m = td.EDMUnet2D(**cfg, dtype=dt).load_state_dict(sd)
    hs.append(sha(m(x, torch.tensor([0.3, 1.1, 1.4]), [c])))
    m.close()
print("tiny attention U-Net fp32 / bf16 / fp16", hs)

sd = _ae_twin.synth_ae_state_dict(_ae_twin.TINY, seed=77)
xa = torch.from_numpy(rng.standard_normal(11, (3, 2, 16, 16))).cuda()
hs = []
for dt in ("fp32", "bf16", "fp16"):
    m = td.EDMAutoencoder(**_ae_twin.TINY, dtype=dt).load_state_dict(sd)
    means, logvars = m.preencode(xa)
    hs.append(sha(means, logvars, m.decode(means)))
    m.close()
print("TINY autoencoder preencode + decode fp32 / bf16 / fp16", hs)

cfg = tiny_config(64, 1)
m = td.EDMUnet2D(**cfg, dtype="bf16").load_state_dict(synth_state_dict(cfg, seed=77))
xs = (torch.from_numpy(rng.standard_normal(12, (2, 5, 16, 16))) * 80.0).cuda().contiguous()
cond = m.cond_rows([torch.from_numpy(rng.standard_normal(13, (2, 58))).cuda()], 2, "cuda")
sig = schedule.karras_sigmas(3)[0].contiguous()
check(lib().td_sample_edm(m._h, 2, 16, 16, 3, ptr(sig), 0.5, ptr(cond), ptr(xs)))
torch.cuda.synchronize()
print("td_sample_edm 3 steps", [sha(xs)])

# ---- the entry points whose staging lives in the call scope of csrc/engine.hip and that nothing above reaches: host buffers on every side
import ctypes as C
import numpy as np
from terrain_diffusion_amd._lib import EdmExt, GridBatch, ae_lib, ae_check
eng = td.engine.get_engine("cuda")
E = eng._h
vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
g = td.EDMUnet2D(**cfg, dtype="bf16").load_state_dict(synth_state_dict(cfg, seed=78))
z = torch.from_numpy(rng.standard_normal(14, (2, 5, 16, 16))).cuda().contiguous()
prev = torch.from_numpy(rng.standard_normal(15, (2, 5, 16, 16))).cuda().contiguous()
out = torch.zeros(2, 5, 16, 16)
check(lib().td_sample_consistency(m._h, 2, 16, 16, 1.1, 0.5, ptr(prev), ptr(z), ptr(cond), ptr(out)))
print("td_sample_consistency, host out", [sha(out)])

org = np.ascontiguousarray(np.array([[0, 0], [0, 8], [8, 0], [8, 8]], dtype=np.int64))
starts, wi, wj = np.array([0, 8], dtype=np.int32), np.array([0, 0, 1, 1], dtype=np.int32), np.array([0, 1, 0, 1], dtype=np.int32)
tiles = torch.zeros(4, 1, 16, 16, device="cuda")
check(lib().td_noise_patches(E, 99, 4, vp(org), 16, 16, 1, 64, 64, 1.5, ptr(tiles)))
canvas = torch.from_numpy(rng.standard_normal(16, (2, 24, 24))).abs().add(1.0).contiguous()
check(lib().td_blend_windows(E, ptr(canvas), 1, 24, 24, 16, 2, vp(starts), 2, vp(starts), 4, vp(wi), vp(wj), ptr(tiles), 1))
norm = torch.zeros(1, 24, 24)
check(lib().td_blend_normalize(E, ptr(canvas), 1, 24, 24, 2.0, ptr(norm)))
print("td_noise_patches + td_blend_windows (host canvas) + td_blend_normalize", [sha(tiles), sha(canvas), sha(norm)])

iy = np.ascontiguousarray(np.array([[min(y // 2, 15), min(y // 2 + 1, 15)] for y in range(24)], dtype=np.int32))
wy = np.ascontiguousarray(np.tile(np.array([0.75, 0.25], dtype=np.float32), (24, 1)))
src, res = torch.from_numpy(rng.standard_normal(17, (1, 16, 16))).contiguous(), torch.zeros(1, 24, 24, device="cuda")
check(lib().td_resample2d(E, ptr(src), 1, 16, 16, 24, 24, vp(iy), vp(wy), 2, vp(iy), vp(wy), 2, ptr(res)))
print("td_resample2d, host input", [sha(res)])

tt = np.arctan(sig[:3].numpy().astype(np.float32) / np.float32(0.5))
cs = np.ascontiguousarray(np.stack([np.cos(tt), np.sin(tt)], 1).astype(np.float32))
xs = (torch.from_numpy(rng.standard_normal(12, (2, 5, 16, 16))) * 80.0).cuda().contiguous()
a = EdmExt(n=2, H=16, W=16, n_steps=3, sigmas_host=ptr(sig), sigma_data=0.5, cond=ptr(cond), x=ptr(xs), cond_img=None, cimg_channels=0, guide=g._h, guidance_scale=1.3,
           score_scaling=0.9, score_cs_host=vp(cs))
check(lib().td_sample_edm_ext(m._h, C.byref(a)))
torch.cuda.synchronize()
print("td_sample_edm_ext, guide + score scaling", [sha(xs)])

means, stds = np.linspace(-0.5, 0.5, 7).astype(np.float32), np.linspace(0.5, 1.5, 7).astype(np.float32)
hist = np.array([0.11, -0.42, 0.93, 0.27, -0.08], dtype=np.float32)
pos = np.ascontiguousarray(np.array([[0, 0], [0, 1], [1, 0], [1, 1]], dtype=np.int32))
grid = torch.from_numpy(rng.standard_normal(18, (7, 5, 5))).contiguous()    # a host grid: the rows are staged
canvas, wins = torch.zeros(6, 24, 24, device="cuda"), torch.zeros(4, 5, 16, 16, device="cuda")
b = GridBatch(noise_seed=99, n=4, H=16, W=16, tile_h=64, tile_w=64, noise_scale=float(sig[0]), origins_host=vp(org), n_steps=3, sigma_data=0.5, sigmas_host=ptr(sig),
              canvas=ptr(canvas), Hc=24, Wc=24, size=16, n_rows=2, n_cols=2, accumulate=1, row_starts_host=vp(starts), col_starts_host=vp(starts), wi_host=vp(wi),
              wj_host=vp(wj), windows_out=ptr(wins), cond_grid=ptr(grid), grid_rows=5, grid_cols=5, cond_pos_host=vp(pos), cond_means_host=vp(means),
              cond_stds_host=vp(stds), hist_host=vp(hist), n_hist=5, noise_level=0.3)
check(lib().td_sample_grid_batch(m._h, C.byref(b)))
torch.cuda.synchronize()
print("td_sample_grid_batch, host grid", [sha(canvas), sha(wins)])

ae = td.EDMAutoencoder(**_ae_twin.TINY, dtype="bf16").load_state_dict(sd)
xh = torch.from_numpy(rng.standard_normal(19, (1, 2, 16, 16))).contiguous()
mu, lv, pk = torch.zeros(1, 3, 8, 8, device="cuda"), torch.zeros(1, 3, 8, 8, device="cuda"), torch.zeros(1, 6, 8, 8, dtype=torch.float16)
ae_check(ae_lib().td_ae_preencode(ae._h, 1, 16, 16, ptr(xh), 0.0, 1.0, 0, ptr(mu), ptr(lv), ptr(pk)))
print("td_ae_preencode, host x and packed_f16", [sha(mu, lv), sha(pk)])

# profile mode: the label set and launch counts of one sampler call and one autoencoder round trip
eng.set_option("profile", 1)
eng.profile_read(reset=True)
xs = (torch.from_numpy(rng.standard_normal(12, (2, 5, 16, 16))) * 80.0).cuda().contiguous()
check(lib().td_sample_edm(m._h, 2, 16, 16, 3, ptr(sig), 0.5, ptr(cond), ptr(xs)))
mu, lv = ae.preencode(xa[:1])
ae.decode(mu)
buf = C.create_string_buffer(1 << 20)
check(lib().td_engine_profile_dump(E, buf, len(buf)))
eng.set_option("profile", 0)
rows = [l.split("\t") for l in buf.value.decode().splitlines()]
print("profile labels", len(rows), "launches", sum(int(r[2]) for r in rows), [hashlib.sha256("\n".join(f"{r[0]} {r[2]}" for r in rows).encode()).hexdigest()[:16]], "sampler", [sha(xs)])
for mod in (m, g, ae):
    mod.close()
