"""Record what ``StripContext`` plans for one rank: halo, messages and the halo-free cut, over a grid of heights and worlds.

    python tests/golden/make_golden_strip_plan.py [output directory, default: this one]

Every case builds ``StripContext(matcher, H, 4, rank, world, "cpu")`` through the public constructor, without a process
group and with a ``types.SimpleNamespace`` for the matcher (``winSize``, and ``alternate`` for the last kind): no GPU, no
native library.  The grid holds empty strips (more ranks than rows), strips thinner than the halo and ranks with a halo on
one side only.  The committed ``strip_plan_cases.json`` was written at the commit BEFORE the plan moved out of
``StripContext.__init__``; ``tests/test_strips_plan_properties.py`` replays the grid and wants every row back.
"""
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

GRID = {"H": [1, 2, 10, 37, 96, 135, 1080], "world": [1, 2, 3, 8],
        "matcher": [{"winSize": 1}, {"winSize": 3}, {"winSize": 11}, {"winSize": 35}, {"winSize": 35, "alternate": True}]}
FIELDS = ("pad", "r0", "r1", "h0", "h1", "top", "bot", "interior", "rows_max", "sends", "recvs")


def replay(grid):
    """One row ``[H, world, rank, matcher index, *FIELDS]`` per case, in grid order."""
    from simplestereo_amd import strips
    rows = []
    for H in grid["H"]:
        for world in grid["world"]:
            for rank in range(world):
                for k, m in enumerate(grid["matcher"]):
                    ctx = strips.StripContext(types.SimpleNamespace(**m), H, 4, rank, world, "cpu")
                    got = [getattr(ctx, f) for f in FIELDS]
                    rows.append([H, world, rank, k] + [[list(t) for t in v] if isinstance(v, list) else int(v) for v in got])
    return rows


def main(out_dir):
    rows = replay(GRID)
    with open(os.path.join(out_dir, "strip_plan_cases.json"), "w") as f:
        f.write('{"grid": %s,\n "fields": %s,\n "rows": [\n' % (json.dumps(GRID), json.dumps(FIELDS)))
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n]}\n")
    print(len(rows), "cases,", sum(r[4 + FIELDS.index("r0")] == r[4 + FIELDS.index("r1")] for r in rows), "with an empty strip")


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else HERE)
