"""Dev tool: per-user band statistics of the top-k workspace, read at
ip_ws_layout's offsets after a scan:
  * the append lists (acnt): entries per list, and how many lists run past
    64 / 128 / 192 / 256 entries (the refine's first window, REFINE_LW);
  * the list-bound band the refine compacts from those lists (entries >= the
    scan's list bound lb - 2 eps, rounded down as round_down_sub does);
  * the theta-band of ip_select_kernel (entries >= theta - 2 eps), built by
    forcing the band through ip_topk_bound.
Usage: python3 tools/band_stats.py D USERS ITEMS [K]"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "news-recommendation-tc_amd"), REPO]
import torch  # noqa: E402

from nrk import ops  # noqa: E402

D, U, I = (int(x) for x in sys.argv[1:4])
K = int(sys.argv[4]) if len(sys.argv) > 4 else 31
g = torch.Generator(device="cuda").manual_seed(5)
users = torch.nn.functional.normalize(torch.randn(U, D, device="cuda", generator=g), dim=1).contiguous()
items = torch.nn.functional.normalize(torch.randn(I, D, device="cuda", generator=g), dim=1).contiguous()
cat = ops.Catalog(items)
ws = ops.ip_topk_workspace(U, cat, K, "cuda")
ops.ip_topk_screen(users, cat, K, ws)
torch.cuda.synchronize()


def a256(x):
    return (x + 255) // 256 * 256


bandcap = min(288, max(96, (2 * K + 32 + 31) // 32 * 32))
o_ucut = 256
o_cnt = o_ucut + a256(U * 8)
o_ovf = o_cnt + a256(U * 4)
o_ovl = o_ovf + a256(U * 4)
o_uinfo = o_ovl + a256(U * 4)
o_acnt = o_uinfo + a256(U * 16)
o_cand = o_acnt + a256(U * 8)
o_app = o_cand + a256(U * bandcap * 8)
app_end = ws.numel() - a256(U * 4) - a256(min(U, 256) * I * 4)  # before the exact path's scratch and slow list
m2 = (app_end - o_app) // (U * 16)
uinfo = ws[o_uinfo:o_uinfo + U * 16].view(torch.float32).view(U, 4)
acnt = ws[o_acnt:o_acnt + U * 8].view(torch.int32).view(U, 2)
q = torch.tensor([0.1, 0.5, 0.9, 0.99, 0.999], device="cuda")
per_list = acnt.reshape(-1).float()
print(f"D={D} U={U} I={I} K={K}: m2 {m2}, band slots {bandcap}")
print(f"  append-list entries per list: mean {per_list.mean():.1f} q10/50/90/99/99.9 {per_list.quantile(q).tolist()} "
      f"max {int(per_list.max())}")
for w in (64, 128, 192, 256):
    print(f"    lists past {w}: {(per_list > w).float().mean():.5f}; users with one: "
          f"{(acnt > w).any(1).float().mean():.5f}")
print(f"  users whose appends overflowed (acnt > m2): {int((acnt > m2).any(1).sum())}")

# the list-bound band: entries >= round_down_sub(lb, 2 eps_s), lb = -inf: all
app = ws[o_app:o_app + U * 2 * m2 * 8].view(torch.int32).view(U, 2, m2, 2)
lb, eps_s = uinfo[:, 0], uinfo[:, 1]
c = lb - 2.0 * eps_s
cut = torch.where(torch.isinf(lb), lb, torch.nextafter(c, torch.full_like(c, float("-inf"))))
band = torch.zeros(U, device="cuda")
slot = torch.arange(m2, device="cuda")
for u0 in range(0, U, 16384):
    u1 = min(U, u0 + 16384)
    v = app[u0:u1, :, :, 0].view(torch.float32)
    live = slot[None, None, :] < acnt[u0:u1].clamp(max=m2)[:, :, None]
    band[u0:u1] = (live & (v >= cut[u0:u1, None, None])).sum((1, 2)).float()
print(f"  list-bound band (the refine's) half-blocks: mean {band.mean():.2f} q {band.quantile(q).tolist()} "
      f"max {int(band.max())}")

# the theta-band: ip_topk_bound runs ip_select_kernel on the same lists
ops.ip_topk_bound(users, cat, K, 1, ws)
torch.cuda.synchronize()
cnt = ws[o_cnt:o_cnt + U * 4].view(torch.int32).float()
ucut = ws[o_ucut:o_ucut + U * 8].view(torch.float32).view(U, 2)
print(f"  theta-band (ip_select_kernel) half-blocks: mean {cnt.mean():.2f} q {cnt.quantile(q).tolist()}")
print(f"  uinfo mean (lb, eps scaled, scale, eps) {uinfo.mean(0).tolist()}; ucut mean {ucut.mean(0).tolist()}")
