"""Writes tests/golden/exrw: for each small case of tests/exrw_util.golden_cases, the input as a
.npy, the file the reference's tinyexr writes for it (SaveEXRToMemory through
oracle/_ref/libref_exr.so, which `make -C oracle ref` builds where the reference is present), and
a manifest. The committed files are data the reference's program wrote; run this only to add cases.

    python3 tools/make_exr_write_goldens.py
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exrw_util as U  # noqa: E402


def ref_save(a, fp16):
    """tinyexr's SaveEXRToMemory(float*, w, h, components, fp16) -> the file's bytes."""
    L = C.CDLL(U.REFLIB)
    L.SaveEXRToMemory.restype = C.c_int
    L.SaveEXRToMemory.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                  C.POINTER(C.c_char_p)]
    a = np.ascontiguousarray(a, np.float32)
    h, w, c = a.shape
    buf, err = C.c_void_p(), C.c_char_p()
    n = L.SaveEXRToMemory(a.ctypes.data, w, h, c, 1 if fp16 else 0, C.byref(buf), C.byref(err))
    if n <= 0:
        raise RuntimeError(f"SaveEXRToMemory -> {n}")
    return C.string_at(buf.value, n)


def main():
    os.makedirs(U.GOLD, exist_ok=True)
    man = {}
    for name, (make, fp16) in U.golden_cases().items():
        a = make()
        np.save(os.path.join(U.GOLD, name + ".npy"), a)
        data = ref_save(a, fp16)
        open(os.path.join(U.GOLD, name + ".exr"), "wb").write(data)
        h, w, c = a.shape
        man[name] = {"input": name + ".npy", "file": name + ".exr", "fp16": int(fp16), "width": w, "height": h,
                     "components": c, "bytes": len(data)}
    json.dump(man, open(os.path.join(U.GOLD, "manifest.json"), "w"), indent=1, sort_keys=True)
    print(json.dumps({k: v["bytes"] for k, v in man.items()}))


if __name__ == "__main__":
    main()
