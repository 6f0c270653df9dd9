"""Two data-parallel ranks sharing cuda:0 over gloo, launched by tests/test_gpu_ema.py through torch.distributed.run: three steps of
FusedAdamW(ema_decay=...) under the sharded optimiser against the same three steps of one rank alone.  Both ranks write the SAME
seeded gradient into the flat buffer, so the reduced gradient times grad_scale = 1/2 is that gradient exactly and the two runs
must agree bit for bit.  A rank's ema is current for its own stripes only (the rest is poisoned with NaN here): ema_weights()
gathers the stripes before it swaps them in.  Writes per rank what it compared."""
import faulthandler, os, sys
faulthandler.dump_traceback_later(int(os.environ.get("D2R_PROBE_DUMP_S", "150")), exit=True)  # a hang ends in tracebacks, not silence
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import torch.distributed as dist

out_dir = sys.argv[1]
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
torch.cuda.set_device(0)
dist.init_process_group("gloo")
assert world == 2, world
from d2r_amd import modules as M
from d2r_amd.config import TextConfig, VisionConfig, default_args
from d2r_amd.dp import DataParallel
from d2r_amd.params import FusedAdamW, ParamStore

dev = torch.device("cuda:0")
DECAY, STEPS = 0.9, 3


def make():
    torch.manual_seed(100)  # the same replica everywhere: the one-rank run starts from the weights the two ranks start from
    tc = TextConfig(num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    vc = VisionConfig(num_hidden_layers=1, image_size=64, patch_size=32)
    model = M.UnimoModelF(default_args(DR_step=3), vc, tc).to(dev)
    model.set_compute_dtype(torch.bfloat16).train()
    store = ParamStore(model, torch.bfloat16)
    return model, store, FusedAdamW(store, lr=1e-3, max_grad_norm=None, ema_decay=DECAY)


model, store, opt = make()
gen = torch.Generator().manual_seed(17)
grads = [(torch.randn(store.n, generator=gen) * 1e-3).to(dev) for _ in range(STEPS)]
# one rank alone
for G in grads:
    store.flat_g.copy_(G)
    opt.step()
torch.cuda.synchronize()
one = dict(w=store.flat_w.clone(), ema=opt.ema.clone())
with opt.ema_weights():
    one["ema_lp"] = store.flat_lp.clone()
del model, store, opt

# two ranks, sharded optimiser; buckets of an odd length: several stripes per rank and a tail in the last bucket
model, store, opt = make()
dp = DataParallel(store, opt, model, bucket_elems=3_000_017, shard_optimizer=True)
assert dp.active and dp.world == 2 and opt.element_ranges is not None
dp.broadcast_parameters()
opt.ema_reset()
for G in grads:
    dp.begin_step()
    store.flat_g.copy_(G)
    dp.reduce_gradients()
    opt.step()
    dp.gather_parameters()
    opt.zero_grad()
torch.cuda.synchronize()
own = torch.zeros(store.n, dtype=torch.bool, device=dev)
for a, b in opt.element_ranges:
    own[a:b] = True
stale_differs = bool((opt.ema[~own] != one["ema"][~own]).any())  # the other rank's stripes were not updated here ...
opt.ema[~own] = float("nan")                                      # ... and nothing may read them: poisoned before the gather
w_live, lp_live = store.flat_w.clone(), store.flat_lp.clone()
with opt.ema_weights():
    torch.cuda.synchronize()
    ema_in_w = store.flat_w.clone()
    lp_in = store.flat_lp.clone()
torch.cuda.synchronize()
gathered = opt.ema.clone()
other = gathered.clone()
dist.broadcast(other, src=0)
sd = opt.state_dict()
res = dict(same_w_as_one_rank=bool(torch.equal(store.flat_w, one["w"])), live_w_restored=bool(torch.equal(store.flat_w, w_live)),
           live_lp_restored=bool(torch.equal(store.flat_lp, lp_live)), swapped_in_is_one_rank_ema=bool(torch.equal(ema_in_w, one["ema"])),
           lp_follows_swap=bool(torch.equal(lp_in, one["ema_lp"])),
           gathered_is_one_rank_ema=bool(torch.equal(gathered, one["ema"])), same_ranks=bool(torch.equal(other, gathered)),
           state_dict_ema=bool(torch.equal(sd["ema"], one["ema"])), stale_differs=stale_differs,
           moved=bool((one["ema"] != one["w"]).any()), finite=bool(torch.isfinite(gathered).all()),
           owned=int(own.sum()), n=store.n)
print(f"rank {rank}: {res}", flush=True)
torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
dist.barrier()
dist.destroy_process_group()
