"""m355_maps_desc and m355_maps_info (include/de265_mi355x.h) as a C compiler lays them out, against the ctypes mirrors of libde265_amd/capi.py:
sizeof and the offset of every member, and the constants that go with them.  No device."""
import ctypes
import os
import subprocess

from libde265_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"m355_maps_desc": capi.MapsDesc, "m355_maps_info": capi.MapsInfo}
CONSTANTS = {"M355_N_MAPS": capi.N_MAPS, "M355_MAPS_REQUESTS": capi.MAPS_REQUESTS, "M355_PICTURE_LAST": capi.PICTURE_LAST, "M355_MAP_CU": capi.MAP_CU,
             "M355_MAP_QP": capi.MAP_QP, "M355_MAP_TU": capi.MAP_TU, "M355_MAP_INTRA": capi.MAP_INTRA, "M355_MAP_MV": capi.MAP_MV,
             "M355_MAP_REF": capi.MAP_REF, "M355_MAP_SLICE": capi.MAP_SLICE}


def test_structs_match_the_ctypes_mirrors(tmp_path):
    names = [(s, f) for s, mirror in STRUCTS.items() for f, _ in mirror._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"de265_mi355x.h\"\nint main(void){\n"
    src += "".join("printf(\"%%zu\\n\", sizeof(%s));\n" % s for s in STRUCTS)
    src += "".join("printf(\"%%zu\\n\", offsetof(%s, %s));\n" % (s, f) for s, f in names)
    src += "".join("printf(\"%%d\\n\", (int)%s);\n" % c for c in CONSTANTS)
    src += "return 0;}\n"
    exe = str(tmp_path / "maps_layout")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src, text=True, check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:len(STRUCTS)] == [ctypes.sizeof(m) for m in STRUCTS.values()]
    for (s, f), off in zip(names, got[len(STRUCTS):]):
        assert off == getattr(STRUCTS[s], f).offset, "%s.%s" % (s, f)
    assert got[len(STRUCTS) + len(names):] == list(CONSTANTS.values())
    assert ctypes.sizeof(capi.MapsDesc) == 120 and ctypes.sizeof(capi.MapsInfo) == 64
    assert capi.MAP_ELEM_BYTES == tuple(d.itemsize * n for d, n in zip(capi.MAP_DTYPES, capi.MAP_PER_UNIT)) == (4, 1, 1, 1, 8, 4, 2)
