"""The fp32 routing of the convolution entry points across flag combinations, on the host (nothing is launched), against a table
recorded from the library as it stood before the dispatcher moved into csrc/conv_dispatch.hip.

Per descriptor of the grid below: yolo_conv_pick_tile, yolo_conv_workspace_bytes, and what yolo_conv_fwd (no workspace) and
yolo_conv_fwd_ws (a 1-byte and a 2^40-byte workspace) return on fake pointers, with the first 24 bytes of yolo_last_error() where
the call was refused. A call that passes every check ends in YOLO_ERR_LAUNCH, with the runtime's text behind a kernel's name and
not a message of the dispatcher's: such a call is recorded as "reaches the launch", not by its code.

The calls are made in a fresh child process from which the GPUs are hidden, and which makes no call at all if it still sees one:
a descriptor that reaches the launch must find no device to launch on. The child loads the library alone (no torch).

    python tests/test_routes_host.py --record [LIB]     writes tests/golden/conv_routes.json (run once, at the parent commit)
"""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_routes.json")
FAKE = 1 << 20          # a non-null "device pointer"
ERR_LAUNCH = -3
F_RESIDUAL, F_FILTERS_READY, F_SPLIT_BF16, F_SPLIT_WEIGHTS_READY, F_SPLIT_K, F_FILTERS_APPENDED = 1, 4, 8, 16, 32, 64
KERNEL_FLAGS = (F_FILTERS_READY, F_SPLIT_BF16, F_SPLIT_WEIGHTS_READY, F_SPLIT_K, F_FILTERS_APPENDED)

GRID = {
    "n": 2,
    "hw": [[13, 13], [19, 19], [20, 13], [26, 26], [52, 52], [208, 208]],
    "cin_cout": [[32, 64], [128, 256], [512, 1024], [1024, 512], [128, 255], [3, 32], [68, 84]],
    "ksize": [1, 3],
    "stride": [1, 2],
    "tile": [0, 4, 5, 7, 12, 13, 15],
    # every subset of the five kernel flags with at most two of them set
    "flags": [sum(c) for k in (0, 1, 2) for c in itertools.combinations(KERNEL_FLAGS, k)],
    "residual": [0, F_RESIDUAL],
}
ENVS = {"default": {}, "no_winograd": {"YOLO_NO_WINOGRAD": "1"}}


def descriptors():
    """The grid in the order of the table's rows: 18 int32 each, the fields of yolo_conv_desc."""
    for (h, w), (cin, cout), k, s, tile, flags, res in itertools.product(*(GRID[a] for a in (
            "hw", "cin_cout", "ksize", "stride", "tile", "flags", "residual"))):
        #      n          h  w  cin  cout k  s  x_ld               off y_ld off r_ld               off act out dtype flags    tile
        yield (GRID["n"], h, w, cin, cout, k, s, (cin + 3) // 4 * 4, 0, cout, 0, cout if res else 0, 0, 1, 0, 0, flags | res, tile)


def rows(lib_path):
    """One outcome per descriptor: [pick_tile, workspace_bytes, fwd, fwd_ws(1 byte), fwd_ws(2^40 bytes)], a call being "L" where it
    reached the launch and [code, first 24 bytes of the message] where it was refused."""
    lib = C.CDLL(lib_path)
    count = C.c_int(0)
    if lib.hipGetDeviceCount(C.byref(count)) == 0 and count.value > 0:      # (the runtime the library links against)
        sys.exit("test_routes_host: a GPU is visible; no call is made on fake pointers")
    P, D = C.c_void_p, C.c_int32 * 18
    lib.yolo_last_error.restype = C.c_char_p
    lib.yolo_conv_workspace_bytes.restype = C.c_size_t
    lib.yolo_conv_fwd.argtypes = [C.POINTER(D)] + [P] * 8
    lib.yolo_conv_fwd_ws.argtypes = [C.POINTER(D)] + [P] * 7 + [C.c_size_t, P, P]

    def outcome(rc):
        if rc == ERR_LAUNCH:
            return "L"
        assert rc < 0, "a call on fake pointers came back with success"
        return [rc, lib.yolo_last_error()[:24].decode()]

    out = []
    for fields in descriptors():
        d = D(*fields)
        res = FAKE if fields[16] & F_RESIDUAL else None
        out.append([lib.yolo_conv_pick_tile(d), lib.yolo_conv_workspace_bytes(d),
                    outcome(lib.yolo_conv_fwd(d, FAKE, FAKE, FAKE, FAKE, res, FAKE, None, None)),
                    outcome(lib.yolo_conv_fwd_ws(d, FAKE, FAKE, FAKE, FAKE, res, FAKE, FAKE, 1, None, None)),
                    outcome(lib.yolo_conv_fwd_ws(d, FAKE, FAKE, FAKE, FAKE, res, FAKE, FAKE, 1 << 40, None, None))])
    return out


def child_rows(lib_path, env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("YOLO_")}
    e.update(env, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows", lib_path], env=e, check=True, stdout=subprocess.PIPE, text=True)
    return json.loads(run.stdout)


def record(lib_path):
    """The table: every distinct outcome once, and per environment one index into them per descriptor."""
    outcomes, index, table = [], {}, {}
    for name, env in ENVS.items():
        table[name] = [index.setdefault(json.dumps(r), len(index)) for r in child_rows(lib_path, env)]
    outcomes = [json.loads(k) for k in index]
    with open(GOLDEN, "w") as f:
        json.dump({"grid": GRID, "outcomes": outcomes, "rows": table}, f, separators=(",", ":"))
        f.write("\n")
    launched = sum("L" in outcomes[i][2:] for t in table.values() for i in t)
    print(f"{GOLDEN}: {sum(map(len, table.values()))} rows, {len(outcomes)} distinct outcomes, {launched} rows reach a launch")


if __name__ == "__main__":
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(here, "yolo_for_turbines_amd", "libyolo_mi355x.so")
    if sys.argv[1:2] == ["--rows"]:
        json.dump(rows(path), sys.stdout, separators=(",", ":"))
    elif sys.argv[1:2] == ["--record"]:
        record(path)
    else:
        sys.exit(__doc__)
else:
    import pytest

    @pytest.fixture(scope="module")
    def built():
        import __graft_entry__ as g
        g.build()
        from yolo_for_turbines_amd import _lib
        return _lib

    @pytest.fixture(scope="module")
    def golden():
        with open(GOLDEN) as f:
            return json.load(f)

    def test_the_table_is_of_this_grid(golden):
        n = len(list(descriptors()))
        assert golden["grid"] == GRID and n == 6 * 7 * 2 * 2 * 7 * 16 * 2
        assert set(golden["rows"]) == set(ENVS) and all(len(t) == n for t in golden["rows"].values())

    @pytest.mark.parametrize("env", list(ENVS))
    def test_every_row_routes_as_recorded(built, golden, env):
        got = child_rows(built.LIB_PATH, ENVS[env])
        want = [golden["outcomes"][i] for i in golden["rows"][env]]
        assert len(got) == len(want)
        bad = [(d, g, w) for d, g, w in zip(descriptors(), got, want) if g != w]
        assert not bad, f"{len(bad)} of {len(want)} rows moved; the first (descriptor, got, recorded): {bad[0]}"
