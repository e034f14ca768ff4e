"""Static check of the library's ISA (fab_torch_amd/_isa_check.py): no instruction touches a register whose vector-memory load
may still be in flight - the property the hand-counted `s_waitcnt vmcnt(N)` of the stream / ring kernels (stream_r8.h,
spline_r8.h, flow_r8.h, flow_r4.h, flow_device.h) rely on.  Usage: python tools/check_r8_isa.py [object stems ...]
(default: every object of the in-tree build, fab_torch_amd/build/*.o; build first).  No GPU needed."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fab_torch_amd import _isa_check as chk          # noqa: E402

BUILD = os.path.join(ROOT, "fab_torch_amd", "build")
AIS_OBJECTS = ("ais_tile16", "ais_tile16_metropolis", "ais_tile48", "ais_moves")       # (ais_driver holds no kernel)
SPLINE_OBJECTS = ("spline_pack", "spline_tile16", "spline_stream")
DEVICE_OBJECTS = ("flow_kernels",) + AIS_OBJECTS + SPLINE_OBJECTS + ("train_kernels", "reduce_kernels", "resample_scan",
                                                    "resample_emit", "weight_decisions", "generic_kernels", "topk")
ALIASES = {"spline": SPLINE_OBJECTS, "flow": AIS_OBJECTS}


def main():
    stems = sys.argv[1:] or DEVICE_OBJECTS
    stems = [t for s in stems for t in ALIASES.get(s, (s,))]
    rc = 0
    for stem in stems:
        obj = os.path.join(BUILD, stem + ".o")
        if not os.path.exists(obj):
            print(f"{obj}: missing (python -m fab_torch_amd._build)")
            rc = 1
            continue
        res = chk.check_object(obj, verbose=bool(os.environ.get("R8ISA_VERBOSE")))
        n_bad = sum(1 for v in res.values() if v)
        print(f"{stem}: {len(res)} kernels, {n_bad} with findings")
        for k, v in res.items():
            if v:
                print("  ", k[:120])
                for f in v[:8]:
                    print("     ", f)
        rc |= bool(n_bad)
    return rc


if __name__ == "__main__":
    sys.exit(main())
