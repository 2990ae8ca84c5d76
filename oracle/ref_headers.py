"""List every function the reference's layers/, signal/ and train/ headers declare, as sorted JSON.

`make -C oracle ref` writes the list to tests/golden/ref_header_functions.json, which the drop-in completeness test
(tests/test_abi_and_symbols.py) reads: the tests never need the reference tree itself.
usage: python3 oracle/ref_headers.py <reference root>"""
import glob
import json
import os
import re
import sys


def declared_functions(ref_root):
    names = set()
    for sub in ("layers", "signal", "train"):
        for f in glob.glob(os.path.join(ref_root, "nntoolkitcore", sub, "*.h")):
            t = re.sub(r"/\*.*?\*/", "", open(f).read(), flags=re.S)
            t = re.sub(r"//.*", "", t)
            names |= {m.group(1) for m in re.finditer(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", t)}
    return sorted(names - {"defined", "sizeof", "void", "float", "int"})    # typedef'd function pointers: `void (*Name)(...)`


if __name__ == "__main__":
    sys.stdout.write(json.dumps({"header_functions": declared_functions(sys.argv[1])}, indent=1) + "\n")
