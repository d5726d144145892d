#!/usr/bin/env python3
"""Probe every option of liblaser_hip.so through laser_hip_get_option / laser_hip_set_option and print (or write) the result as JSON.

    python scripts/record_options.py                 # print the probe of the built library
    python scripts/record_options.py --write PATH    # record it (tests/golden/options_parent.json was made this way)

For each name the library's source accepts: the return code and value of get_option before anything is set, then for each
probe value the return code of set_option and the value read back; a name stops at its first refusal (a read-only diagnostic
refuses at once) and is put back to its first value.  No call needs a device, so this runs on a machine without a GPU; run it in a
process that has not used the library yet (tests/test_options_cpu.py starts it as a child), because the diagnostics are process state.
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROBES = [-70000, -3, -2, -1, 0, 1, 2, 3, 4, 5, 9, 10, 64, 65, 65535, 65536, 2147483647]
CAPI = os.path.join(ROOT, "laser_amd", "csrc", "capi.cpp")


def option_names(text=None):
    """The names capi.cpp accepts, in source order: the rows of its option table (`{"name", ...`), or -- before there was a table --
    the quoted names of the two `n == "name"` chains."""
    if text is None:
        text = open(CAPI).read()
    names = re.findall(r'^\s*\{"(\w+)"|\bn == "(\w+)"', text, re.M)
    return list(dict.fromkeys(a or b for a, b in names))


def probe(names=None):
    import ctypes as C
    import laser_amd
    L = laser_amd.lib()

    def get(name):
        v = C.c_int64(0)
        rc = L.laser_hip_get_option(name.encode(), C.byref(v))
        return [rc, int(v.value) if rc == 0 else None]

    names = option_names() if names is None else names
    out = {n: {"get": get(n), "set": []} for n in names}     # every first read before any write
    for n in names:
        first = out[n]["get"]
        try:
            for p in PROBES:
                rc = L.laser_hip_set_option(n.encode(), p)
                out[n]["set"].append([p, rc, get(n)[1] if rc == 0 else None])
                if rc != 0:
                    break
        finally:
            if first[0] == 0 and out[n]["set"] and out[n]["set"][0][1] == 0:
                L.laser_hip_set_option(n.encode(), first[1])
                out[n]["restored"] = get(n) == first
    return out


if __name__ == "__main__":
    result = probe()
    text = json.dumps(result, indent=1, sort_keys=True) + "\n"
    if len(sys.argv) == 3 and sys.argv[1] == "--write":
        open(sys.argv[2], "w").write(text)
        writable = sum(1 for r in result.values() if r["set"] and r["set"][0][1] == 0)
        print(f"{len(result)} names, {writable} writable, every writable one restored: "
              f"{all(r.get('restored', True) for r in result.values())}")
    else:
        sys.stdout.write(text)
