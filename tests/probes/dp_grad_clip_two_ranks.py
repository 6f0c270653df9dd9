"""Two data-parallel ranks sharing cuda:0 over gloo, launched by tests/test_gpu_grad_clip.py through torch.distributed.run: three
steps of FusedAdamW(max_grad_norm=...) with a norm small enough that every step clips, once with the bucketed all-reduce and once
with the sharded optimiser (each rank sums its own stripes, the bucket tails are counted on rank 0 only, the partial sums are
all-gathered).  Writes per rank the fp64 total of every step, the fp32 norms and coefficients and the final weights."""
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
from d2r_amd.dp import DataParallel, shard_batch
from d2r_amd.params import FusedAdamW, LinearWarmupSchedule, ParamStore

dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(3)
ids = torch.randint(1000, 30000, (4, 16), generator=g); ids[:, 0] = 101
full = (ids, torch.ones(4, 16, dtype=torch.long), torch.zeros(4, 16, dtype=torch.long), torch.randint(0, 3, (4,), generator=g),
        torch.randn(4, 3, 64, 64, generator=g))
batch = tuple(t.to(dev) for t in shard_batch(full, rank, world))
res = {}
for mode, kw in (("all_reduce", {}), ("shard", dict(shard_optimizer=True))):
    torch.manual_seed(100 + rank)  # different replicas on purpose: broadcast_parameters must make them identical
    tc = TextConfig(num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    vc = VisionConfig(num_hidden_layers=1, image_size=64, patch_size=32)
    model = M.UnimoModelF(default_args(DR_step=3), vc, tc).to(dev)
    model.set_compute_dtype(torch.bfloat16).train()
    model.model.use_streams = False
    store = ParamStore(model, torch.bfloat16)
    opt = FusedAdamW(store, lr=1e-3, max_grad_norm=1e-3)
    sched = LinearWarmupSchedule(opt, 0, 12)
    # buckets of an odd length: several stripes per rank and a tail in the last bucket
    dp = DataParallel(store, opt, model, bucket_elems=3_000_017, **kw)
    assert dp.active and dp.world == 2
    dp.reducer.poison_stale = True  # sharded: the stripes a rank does not own hold NaN - the norm must not read them
    dp.broadcast_parameters()
    totals, norms, coefs = [], [], []
    for _ in range(3):
        dp.begin_step()
        loss, _ = model(*batch)
        loss.backward()
        dp.reduce_gradients()
        opt.step()
        dp.gather_parameters()
        sched.step()
        opt.zero_grad()
        torch.cuda.synchronize()
        cb = opt._clip
        totals.append(float(cb["slab_all"].sum()) * (opt.grad_scale ** 2))  # the squared norm of the averaged gradient, fp64
        norms.append(float(cb["out"][0]))
        coefs.append(float(cb["out"][1]))
    w = store.flat_w.detach().clone()
    other = w.clone()
    dist.broadcast(other, src=0)
    res[mode] = dict(totals=totals, norms=norms, coefs=coefs, same_ranks=bool(torch.equal(other, w)),
                     finite=bool(torch.isfinite(w).all()), nseg=opt._clip["nseg"], gathered=opt._clip["slab_all"].numel())
    print(f"rank {rank} {mode}: norms {norms} coefs {coefs}", flush=True)
torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
dist.barrier()
dist.destroy_process_group()
