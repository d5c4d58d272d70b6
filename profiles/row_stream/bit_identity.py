"""One fixed list of calls through every kernel of the row family; writes a sha256 of each result's raw
bytes. Run from the root of a built tree: python profiles/row_stream/bit_identity.py OUT.json
(for two trees: once in each, then compare the two files)."""
import hashlib
import json
import math
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from cuda_mpi_reductions_amd.ops import arg_reduce, fill_, reduce_dim  # noqa: E402
from cuda_mpi_reductions_amd.ops.reduce_many import ReduceMany  # noqa: E402

res = {}


def digest(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.reshape(-1).contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def make(shape, dt, misalign=0, seed=1):
    n = math.prod(shape)
    base = torch.empty(n + misalign, dtype=dt, device="cuda")
    fill_(base, "uniform" if dt.is_floating_point else "fullrange", seed=seed)
    if not dt.is_floating_point:
        base.remainder_(1 << 20)
    return base[misalign:].view(shape)


def record(name, fn):
    try:
        out = fn()
        if isinstance(out, (tuple, list)):
            res[name] = [digest(o) for o in out]
        else:
            res[name] = digest(out)
    except (ValueError, TypeError) as e:  # the Python layer's argument checks: the same in both trees
        res[name] = "error: " + str(e)[:80]
    except RuntimeError as e:
        if "unsupported" not in str(e):
            raise  # anything else (a GPU fault above all) ends the job
        res[name] = "error: " + str(e)[:80]


DIM_ROWS = [("long_split", (2, 4_000_037), 0), ("long_split_mis", (3, 1_000_003), 1), ("long_unsplit", (5000, 5000), 0),
            ("long_unsplit_mis", (4999, 5001), 1), ("short_aligned", (100_003, 64), 0), ("short_aligned8", (300_001, 8), 0),
            ("short_mis", (100_003, 17), 0), ("short_mis_base", (50_000, 64), 1)]
DIM_COLS = [("cols_vec", (5000, 512), 0), ("cols_scalar", (5000, 77), 0), ("cols_scalar_mis", (3000, 512), 1),
            ("cols_split", (100_003, 8), 0), ("cols_split_scalar", (100_003, 3), 0)]


def arg_cases(es):  # the vector variants go by the row's bytes: <= 1024 one, <= 2048 two, <= 4096 four vectors per lane
    return [("arg_long_whole", (1, 3_000_001), 0), ("arg_long_rows", (300, 100_001), 0), ("arg_long_split_rows", (8, 2_000_003), 1),
            ("arg_wave", (1000, 3000), 0), ("arg_wave_mis", (999, 3001), 1), ("arg_vec1", (50_000, 512 // es), 0),
            ("arg_vec2", (20_000, 1600 // es), 0), ("arg_vec4", (20_000, 3200 // es), 0), ("arg_scalar1", (50_000, 33), 0),
            ("arg_scalar2", (50_000, 77), 1), ("arg_scalar4", (50_000, 200), 1)]


for dt in (torch.float64, torch.bfloat16, torch.int32):
    d = str(dt).replace("torch.", "")
    for op in ("sum", "min", "max"):
        for name, shape, mis in DIM_ROWS:
            x = make(shape, dt, mis, seed=shape[0] + shape[1])
            record(f"{d}/{op}/rows/{name}", lambda: reduce_dim(x, op, 1))
            if name.startswith("short_aligned"):
                os.environ["MIREDUCE_DIM_SHORT_PIPE"] = "0"
                record(f"{d}/{op}/rows/{name}/single_batch", lambda: reduce_dim(x, op, 1))
                del os.environ["MIREDUCE_DIM_SHORT_PIPE"]
        for name, shape, mis in DIM_COLS:
            x = make(shape, dt, mis, seed=shape[0] * 3 + shape[1])
            record(f"{d}/{op}/cols/{name}", lambda: reduce_dim(x, op, 0))
        ts = [make((n,), dt, mis, seed=n) for n, mis in ((1, 0), (1000, 1), (100_003, 0), (3_000_001, 1), (65_536, 0), (12_345_678, 0))]
        record(f"{d}/{op}/many", lambda: ReduceMany(ts, op)().clone())
    record(f"{d}/sumsq/many", lambda: ReduceMany(ts, "sumsq")().clone())
    for op in ("max", "min"):
        for name, shape, mis in arg_cases(torch.empty((), dtype=dt).element_size()):
            x = make(shape, dt, mis, seed=shape[0] * 5 + shape[1])
            if name == "arg_long_whole":
                record(f"{d}/{op}/{name}", lambda: arg_reduce(x.view(-1), op))
            else:
                record(f"{d}/{op}/{name}", lambda: arg_reduce(x, op, 1))

os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
json.dump(res, open(sys.argv[1], "w"), indent=0, sort_keys=True)
print(f"bitident: {len(res)} calls, {sum(1 for v in res.values() if isinstance(v, str) and v.startswith('error'))} errors")
