"""CPU launch trace of one FusedAdamW.step() on 130 CPU tensors in two param groups, recorded with the recorder of
tests/launch_trace.py: which entry points the optimizer reaches, how many launches (per group: the prepare launches +
ceil(n / 64) update launches) and with which scalar arguments - the learning rate travels by value in eager mode, the lr_dev
argument is null.  The fixture lives in its own directory, tests/golden/launch_traces_optim/ (launch_trace.py's CASES and directory
stay as they are: tools/attn_select_fixture.py and tools/rows_select_fixture.py enumerate every file there);
`python tests/launch_trace_optim.py` rewrites it."""
import gzip
import json
import os

import torch

import launch_trace as lt
from cobevt_amd import host

FIXTURES = os.path.join(lt.ROOT, "tests", "golden", "launch_traces_optim")
CASE = "fused_adamw_step_130"
# (tensors, elements of tensor i, lr, weight_decay, eps) per param group; tensor 7 of group 0 has no gradient
GROUPS = ((100, lambda i: 1 + 37 * i, 2e-4, 1e-2, 1e-10), (30, lambda i: 4096 * (i % 3) + 5, 1e-3, 0.0, 1e-8))
NO_GRAD = 7


def build():
    torch.manual_seed(0)
    groups = []
    for n, size, lr, wd, eps in GROUPS:
        params = [torch.nn.Parameter(torch.zeros(size(i))) for i in range(n)]
        for p in params:
            p.grad = torch.ones_like(p)
        groups.append({"params": params, "lr": lr, "weight_decay": wd, "eps": eps})
    groups[0]["params"][NO_GRAD].grad = None
    return host.FusedAdamW(groups, betas=(0.9, 0.999))


def trace(setattr_):
    rec = lt.Recorder()
    lt.install(setattr_, rec)
    build().step()
    return rec.records


def fixture_path():
    return os.path.join(FIXTURES, CASE + ".jsonl.gz")


def read_fixture():
    with gzip.open(fixture_path(), "rt") as f:
        return [json.loads(line) for line in f]


if __name__ == "__main__":
    os.makedirs(FIXTURES, exist_ok=True)
    first = lt.dumps(trace(setattr))
    if lt.dumps(trace(setattr)) != first:
        raise SystemExit("%s: two runs gave different traces" % CASE)
    with open(fixture_path(), "wb") as f:
        f.write(gzip.compress(first.encode(), mtime=0))
    print("%-44s %5d launches  %7d bytes" % (CASE, first.count("\n"), len(first)))
