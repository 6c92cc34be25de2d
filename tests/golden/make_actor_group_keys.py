"""Records actor_group_store_keys.json: the rendezvous-store keys an actor touches when it joins the
trainer's "actor" weight-update group (gloo, world 2, rank 1) through the REFERENCE's group helper
(pipelinerl/torch_utils.py init_extra_process_group), the trainer side being this project's
WeightUpdateManager as in tests/test_weight_update_cpu.py.  The output is a data fixture.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_actor_group_keys.py <reference checkout>
"""

import json
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import torch  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

from test_weight_update_cpu import _run, free_port  # noqa: E402

if __name__ == "__main__":
    reference = str(Path(sys.argv[1]).resolve())
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_run, args=(free_port(), 2, "per_tensor", tmp, reference), nprocs=2, join=True)
        keys = json.loads((Path(tmp) / "actor0_keys.json").read_text())
    out = {"what": "sorted 'op key' notes of the store behind the reference helper's PrefixStore, actor rank",
           "group_name": "actor", "backend": "gloo", "world_size": 2, "rank": 1, "torch": torch.__version__,
           "keys": keys}
    (HERE / "actor_group_store_keys.json").write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out, indent=1))
