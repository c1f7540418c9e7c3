"""What the host tests of the C ABI share (a helper module like guarded.py: no settings, one fixture to import): the parser
of a public header, the library's exported symbols, and the `lib` fixture that rebuilds a stale library before loading it."""
import re
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
INCLUDE = REPO / "include"
CSRC = REPO / "molecular_dynamics_neural_operator_amd" / "csrc"
DECLARATION = r"^(?:int|size_t|const char\*)\s+(mdno\w+)\s*\(([^;]*?)\)\s*;"


def declared_functions(header_path):
    """name -> number of parameters, for every function a header declares (comments stripped first)."""
    text = re.sub(r"/\*.*?\*/", "", Path(header_path).read_text(), flags=re.S)
    decls = {}
    for m in re.finditer(DECLARATION, text, flags=re.S | re.M):
        args = m.group(2).strip()
        decls[m.group(1)] = 0 if args in ("", "void") else len([a for a in args.split(",") if a.strip()])
    return decls


def exported_symbols():
    """The defined text symbols of the library's dynamic table."""
    from molecular_dynamics_neural_operator_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if " T " in l}


def built_library():
    """The loaded library, rebuilt first where it is missing or its stamp is not the tree's id."""
    from molecular_dynamics_neural_operator_amd import _lib
    stamp = CSRC / "build" / "BUILD_ID"
    if not _lib.LIB_PATH.exists() or not stamp.exists() or stamp.read_text().split()[0] != _lib.source_build_id():
        import __graft_entry__ as g      # (build.sh rebuilds everything when the sources' content hash moved)
        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def lib():
    return built_library()
