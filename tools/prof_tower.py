"""Run only the bench's config-2 user-tower call a few times (profiling driver,
dev tool): REPS launches of ops.tt_user_fwd over 250,000 users, T = 30,
h0 = 64, D = 32.  CHECK=1 also compares the rows with the layers kernel."""
import os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "news-recommendation-tc_amd"), REPO]
import torch
import bench
from nrk import ops

dev = torch.device("cuda", 0)
U, I, D = int(os.environ.get("U", 250000)), 364047, 32
wl = bench.recall_workload(23, U, I, D, dev)
args = (wl["user_table"], wl["item_table"], wl["uid"], wl["hist"], wl["hist_len"])
out = torch.empty((U, D), dtype=torch.float32, device=dev)
for _ in range(int(os.environ.get("REPS", 10))):
    ops.tt_user_fwd(*args, wl["w0"], wl["b0"], wl["w1"], wl["b1"], validate=False, out=out)
torch.cuda.synchronize()
if os.environ.get("CHECK"):
    ref = ops.tt_user_fwd_layers(*args, [(wl["w0"], wl["b0"]), (wl["w1"], wl["b1"])])
    print("rows equal to the layers kernel:", bool(torch.equal(out, ref)))
print("mean history length %.2f" % float(wl["hist_len"].float().mean()))
print("done")
