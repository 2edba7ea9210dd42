"""Worker body of the two-rank derived-quantities test (spawned by torch.multiprocessing from tests/test_hipcallbacks_derived.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

D, K = 4, 2
CASES = [dict(resample=r, trim_importance_weights=t) for r in (False, True) for t in (True, False)]


def derived_gpu_worker(rank, world, port, out_dir, base, derived):
    """2 ranks sharing cuda:0 over gloo: the same sharded run with and without derived() in the source; every posterior array of
    both goes to a file per rank for the parent to compare."""
    import json
    import numpy as np
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import tempest_amd as tp
    out, rows = {}, []
    for tag, cb in (("plain_", tp.HipCallbacks(base, D)), ("", tp.HipCallbacks(base + derived, D, n_derived=K))):
        s = tp.Sampler(cb.prior_transform, cb.log_likelihood, D, n_particles=512, vectorize=True, clustering=False,
                       random_state=4, device=0)
        assert s.state.comm is not None and s._core.n_local == 256
        s.run(n_total=2048, progress=False)
        assert len(s.posterior()) == 3
        for i, case in enumerate(CASES):
            np.random.seed(3)                  # resample=True draws its offset from NumPy's global stream: the same on every rank
            res = s.posterior(return_blobs=True, **case)
            assert len(res) == (4 if tag == "" else 3)
            for key, a in zip(("x", "w", "logl", "blobs"), res):
                out[f"{tag}{key}{i}"] = a
            if tag == "":
                rows.append(int(len(res[0])))
    np.savez(os.path.join(out_dir, f"derived{rank}.npz"), **out)
    json.dump({"cases": len(CASES), "rows": rows}, open(os.path.join(out_dir, f"derived{rank}.json"), "w"))
    dist.barrier()
    dist.destroy_process_group()
