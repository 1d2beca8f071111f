"""The instantiations of the four hot kernel families (k_conv, k_conv_spec, k_obs_rows, k_obs_blocks) are named in ONE place,
sound-spaces_amd/csrc/ss_dispatch.hpp: the library and the host simulator both reach a kernel through its switches, so a CPU test
runs the instantiation the library runs for the same plan.  Any other file that names one restates that choice - a new site
fails here until it is either routed through the dispatch or added to the allow-list with its reason."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = re.compile(r"ssk::k_(conv|conv_spec|obs_rows|obs_blocks)<")
SOURCE = (".hip", ".hpp", ".cpp", ".h", ".c")

# (file, sites): product code first; under tests/ only drivers that deliberately run an instantiation no plan would produce
ALLOWED = {
    "sound-spaces_amd/csrc/ss_dispatch.hpp": 43,
}


def _sites():
    found = {}
    for top in ("sound-spaces_amd", "include", "tests"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith(SOURCE):
                    path = os.path.join(d, f)
                    with open(path, errors="replace") as fh:
                        n = len(PATTERN.findall(fh.read()))
                    if n:
                        found[os.path.relpath(path, ROOT).replace(os.sep, "/")] = n
    return found


def test_the_instantiations_are_named_in_the_dispatch_header_alone():
    assert _sites() == ALLOWED


def test_the_library_and_the_simulator_include_the_dispatch():
    for rel in ("sound-spaces_amd/csrc/ss_hip.hip", "tests/hostsim/hostsim.cpp"):
        with open(os.path.join(ROOT, rel)) as f:
            text = f.read()
        assert "ss_dispatch.hpp" in text and "ssdispatch::" in text, rel
