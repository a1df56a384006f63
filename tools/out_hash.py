"""sha256 of engine outputs on fixed inputs: compares two builds of the library bit for bit.  The base U-Net at batch 64 / 5 / 1 (bf16); an attention-bearing
tiny U-Net (attention in encoder and decoder blocks, with and without a channel change) at 16 x 16, n = 3, and the TINY autoencoder's preencode + decode,
each in fp32 / bf16 / fp16; one 3-step td_sample_edm call, n = 2, on the tiny U-Net (captured graph, fused solver step under the default options).
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
m.close()
