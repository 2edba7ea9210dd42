"""Worker of the two-rank pointwise test (tests/test_hipcallbacks_pointwise.py starts one fresh process per rank):
python -m tests._dist_workers_pointwise RANK WORLD PORT OUT_DIR."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pointwise_gpu_worker(rank, world, port, out_dir):
    """2 ranks sharing cuda:0 over gloo: a sharded run whose source is pointwise-enabled; Sampler.pointwise refuses on every rank, and
    the run goes on to its posterior."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import tempest_amd as tp
    from tests.test_hipcallbacks_pointwise import TERM_X
    cb = tp.HipCallbacks(TERM_X, 3, n_terms=5, pointwise=True)
    s = tp.Sampler(cb.prior_transform, cb.log_likelihood, 3, n_particles=512, vectorize=True, clustering=False, random_state=4, device=0)
    assert s.state.comm is not None and s._core.n_local == 256
    s.run(n_total=2048, progress=False)
    meta = {"raised": None, "message": "", "finished": False}
    try:
        s.pointwise()
    except NotImplementedError as e:
        meta["raised"], meta["message"] = type(e).__name__, str(e)
    x, w, logl = s.posterior()
    meta["rows"], meta["finished"] = int(len(x)), True
    json.dump(meta, open(os.path.join(out_dir, f"pointwise{rank}.json"), "w"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    pointwise_gpu_worker(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
