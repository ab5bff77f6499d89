"""Forward + backward of the detection-loss table node with every loss KIND at the rv-av2 size (4 sweeps of 64 x 2048, 26 classes in
32-float rows, one entry): VARIFOCAL / L1 on the existing ``rv_detection_loss_multilevel_*`` pair (twice, as two variants: their
difference is the run-to-run spread of this table) and, on the ``rv_detection_loss_table_*`` pair, VARIFOCAL / L1, FOCAL / SMOOTH_L1 and
PENALTY_REDUCED / HUBER.  Variants are interleaved round by round (the order alternates), every forward + backward pair is timed with
HIP events, warm-up rounds are discarded.  Synthetic entry: a grid of rectangular instances over a tenth of the pixels, residuals on both
sides of beta / delta = 0.125, one pixel in twelve of an instance predicted exactly (soft target 1).

    python profiles/tools/ab_loss_kinds.py [--rounds 60] [--warmup 10] > profiles/ab_loss_kinds.txt
"""
import argparse, ctypes, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from range_view_3d_detection_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=60)
ap.add_argument("--warmup", type=int, default=10)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("ab_loss_kinds.py needs an MI355X: there is nothing to time without one")
dev = torch.device("cuda:0")
B, H, W, N_CLS, LD = 4, 64, 2048, 26, 32
g = torch.Generator().manual_seed(0)
pan = torch.zeros((B, H, W), dtype=torch.int64)
labels = torch.full((B, H, W), N_CLS, dtype=torch.int64)
ppo = torch.zeros((B, H, W), dtype=torch.int64)
k = 0
for b in range(B):
    k = 0
    for y in range(0, H, 16):
        for x in range(0, W, 128):
            k += 1
            pan[b, y:y + 5, x:x + 40] = k
            labels[b, y:y + 5, x:x + 40] = k % N_CLS
            ppo[b, y:y + 5, x:x + 40] = 200
inst = pan > 0
rng = 5 + 55 * torch.rand((B, H, W), generator=g)
az = (torch.rand((B, H, W), generator=g) * 2 - 1) * 3.14159
cart = torch.stack([rng * az.cos(), rng * az.sin(), torch.rand((B, H, W), generator=g) - 0.5], dim=1)
tg = (torch.rand((B, 8, H, W), generator=g) * 2 - 1) * inst[:, None]
delta = 0.25 * torch.randn((B, 8, H, W), generator=g) * (torch.rand((B, 1, H, W), generator=g) >= 1 / 12)
reg = torch.where(inst[:, None], tg + delta, torch.randn((B, 8, H, W), generator=g))
logits = torch.zeros((B, H, W, LD))
logits[..., :N_CLS] = 3 * torch.randn((B, H, W, N_CLS), generator=g)
regs = torch.zeros((B, H, W, LD))
regs[..., :8] = reg.permute(0, 2, 3, 1)
mask = (torch.rand((B, H, W), generator=g) > 0.1).to(torch.uint8)
t = {n: v.to(dev).contiguous() for n, v in dict(logits=logits, regs=regs, cart=cart, mask=mask, labels=labels, pan=pan, tg=tg, ppo=ppo).items()}
nobj = torch.tensor([B * k], dtype=torch.int32, device=dev)
soft = torch.empty((B, N_CLS, H, W), device=dev)
fg = torch.empty((B, H, W), device=dev)
d_l, d_r = torch.empty((B, H, W, LD), device=dev), torch.empty((B, H, W, LD), device=dev)
sums = torch.empty((2, L.loss_sums_len()), dtype=torch.float64, device=dev)
table = (L.LossEntry * 1)(L.LossEntry(t["logits"].data_ptr(), t["regs"].data_ptr(), t["cart"].data_ptr(), t["mask"].data_ptr(), t["labels"].data_ptr(), t["pan"].data_ptr(),
                                      t["tg"].data_ptr(), t["ppo"].data_ptr(), nobj.data_ptr(), soft.data_ptr(), fg.data_ptr(), d_l.data_ptr(), d_r.data_ptr(), LD, LD, B, N_CLS, H, W))
ONES = (ctypes.c_float * 8)(*[1.0] * 8)


def params(alpha, gamma):
    return L.LossParams(ONES, 1.0, 1.0, 1.0, 0.75, alpha, gamma, 1)


VARIANTS = {  # name -> (params, kinds or None = the existing pair)
    "varifocal/l1 existing pair (A)": (params(0.75, 2.0), None),
    "varifocal/l1 existing pair (B)": (params(0.75, 2.0), None),
    "varifocal/l1 table pair": (params(0.75, 2.0), L.LossKinds(L.CLS_VARIFOCAL, L.REG_L1, 0.0)),
    "focal/smooth_l1 table pair": (params(0.25, 2.0), L.LossKinds(L.CLS_FOCAL, L.REG_SMOOTH_L1, 0.125)),
    "penalty_reduced/huber table pair": (params(1.0, 2.0), L.LossKinds(L.CLS_PENALTY_REDUCED, L.REG_HUBER, 0.125)),
}


def step(p, kinds):
    st = L.stream_ptr()
    if kinds is None:
        L.call("rv_detection_loss_multilevel_forward", table, 1, ctypes.byref(p), L.ptr(sums), st)
        L.call("rv_detection_loss_multilevel_backward", table, 1, ctypes.byref(p), L.ptr(sums), 1.0, st)
    else:
        L.call("rv_detection_loss_table_forward", table, 1, ctypes.byref(p), ctypes.byref(kinds), None, L.ptr(sums), st)
        L.call("rv_detection_loss_table_backward", table, 1, ctypes.byref(p), ctypes.byref(kinds), None, L.ptr(sums), 1.0, st)


names = list(VARIANTS)
ms = {n: [] for n in names}
loss = {}
for r in range(args.warmup + args.rounds):
    for n in (names if r % 2 == 0 else names[::-1]):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step(*VARIANTS[n])
        e1.record()
        e1.synchronize()
        loss[n] = float(sums[1, 16])
        if r >= args.warmup:
            ms[n].append(1000.0 * e0.elapsed_time(e1))
print(f"# ab_loss_kinds: forward + backward of one table entry, {B} x {H} x {W}, {N_CLS} classes in {LD}-float rows, {args.rounds} rounds after {args.warmup} warm-up,")
print(f"# interleaved, HIP events; device {torch.cuda.get_device_name(0)}; microseconds per forward + backward pair")
print(f"{'variant':36s} {'median':>8s} {'min':>8s} {'p10':>8s} {'p90':>8s} {'vs (A)':>7s}   loss")
base = statistics.median(ms[names[0]])
for n in names:
    v = sorted(ms[n])
    print(f"{n:36s} {statistics.median(v):8.1f} {v[0]:8.1f} {v[int(0.1 * (len(v) - 1))]:8.1f} {v[int(0.9 * (len(v) - 1))]:8.1f} {statistics.median(v) / base:7.3f}   {loss[n]:.6f}")
