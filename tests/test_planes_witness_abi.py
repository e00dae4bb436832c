"""The three entries that lead into and out of the packed digit planes without a step
(lf_dev_pack_planes, lf_dev_planes_witness, lf_dev_planes_check): exported by the library, declared
in include/lf.h, bound in latticeum_amd/_lib.py and on Context, and lf_planes_fault's values. No GPU."""
import re
from pathlib import Path

import latticeum_amd as LA
from latticeum_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("lf_dev_pack_planes", "lf_dev_planes_witness", "lf_dev_planes_check")


def header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include/lf.h").read_text(), flags=re.S)


def test_entries_are_exported_declared_and_bound():
    lib = _lib.load()
    txt = header()
    for name in ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(rf"\bint\s+{name}\s*\(\s*lf_ctx\s*\*", txt), f"{name} is not declared in lf.h"
        assert name in _lib.SIGNATURES, f"{name} has no signature in _lib.py"
    assert len(_lib.SIGNATURES["lf_dev_pack_planes"][1]) == 5
    assert len(_lib.SIGNATURES["lf_dev_planes_witness"][1]) == 7
    assert len(_lib.SIGNATURES["lf_dev_planes_check"][1]) == 8
    for method in ("dev_pack_planes", "dev_planes_witness", "dev_planes_check"):
        assert callable(getattr(LA.Context, method))


def test_fault_enum_values():
    m = re.search(r"enum\s+lf_planes_fault\s*\{([^}]*)\}", header())
    assert m, "enum lf_planes_fault is not in lf.h"
    vals = {k.strip(): int(v) for k, v in (item.split("=") for item in m.group(1).split(","))}
    assert vals == {"LF_PLANES_OK": 0, "LF_PLANES_ENCODING": 1, "LF_PLANES_BOUND": 2}
    assert (LA.PLANES_OK, LA.PLANES_ENCODING, LA.PLANES_BOUND) == (0, 1, 2)
