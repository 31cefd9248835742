"""The step drivers time their stages and kernels by name, through the sim's StepTimer (sx_step_timer.hpp).

The stage and kernel times used to be event arrays indexed by a running counter and by magic numbers: one record too
many or too few moved every later time under the wrong name, and nothing failed.  So sx_sim*.cpp and sx_bdt.cpp hold
no such event array any more; they mark `Stage::X` / `Kernel::X` on the timer, and only the timer turns events into
times.  One timing of its own remains in those files: the turbulence stirring.
"""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(__file__), "..", "sph-exa_amd", "csrc")
STAGES = ["sync", "FindNeighbors", "XMass", "VeDefGradh", "EOS", "IadDivvCurlv", "AVswitches", "MomentumEnergy",
          "Gravity", "UpdateQuantities"]
KERNELS = ["findNeighbors", "xmass", "veDefGradh", "iadDivvCurlv", "avSwitches", "momentumEnergy", "gravity",
           "nbodyIntegrate"]


def driver_sources():
    files = sorted(glob.glob(os.path.join(CSRC, "sx_sim*.cpp"))) + [os.path.join(CSRC, "sx_bdt.cpp")]
    assert len(files) >= 6, files
    out = {}
    for path in files:
        with open(path) as f:
            out[os.path.basename(path)] = f.read()
    return out


def test_no_indexed_stage_or_kernel_events():
    # SimTurb::ev (s->turb->ev[k]) is the stirring's own and stays
    indexed = re.compile(r"(?<!turb)->ev\[|->kev\[|\.ev\+\+|\bkev\b|\+\+\s*ev\b|\bev\+\+")
    marks = 0
    for name, text in driver_sources().items():
        for m in indexed.finditer(text):
            line = text.count("\n", 0, m.start()) + 1
            raise AssertionError("%s:%d: a timing event by index: %r" % (name, line, m.group(0)))
        # the timer's marks name what they mark
        for m in re.finditer(r"\bstageEnd\s*\(\s*([^,]*),", text):
            assert re.fullmatch(r"Stage::\w+", m.group(1).strip()), (name, m.group(0))
            assert m.group(1).strip()[len("Stage::"):] in STAGES, (name, m.group(0))
            marks += 1
        for m in re.finditer(r"\b(?:timer|T)\s*(?:\.|->)\s*(?:begin|end)\s*\(\s*([^,]*),", text):
            assert re.fullmatch(r"Kernel::\w+", m.group(1).strip()), (name, m.group(0))
            assert m.group(1).strip()[len("Kernel::"):] in KERNELS, (name, m.group(0))
            marks += 1
    assert marks > 40, "the patterns no longer find the timer's marks (%d)" % marks


def test_elapsed_time_is_read_by_the_timer_alone():
    with open(os.path.join(CSRC, "sx_step_timer.hpp")) as f:
        timer = f.read()
    assert "hipEventElapsedTime" in timer
    for name, text in driver_sources().items():
        for m in re.finditer(r"hipEventElapsedTime", text):
            line_start = text.rfind("\n", 0, m.start()) + 1
            line = text[line_start:text.index("\n", m.start())]
            assert "turb->" in line, "%s:%d: %s" % (name, text.count("\n", 0, m.start()) + 1, line.strip())
    # every step driver ends in the one collect()
    sources = driver_sources()
    for name in ("sx_sim.cpp", "sx_sim_nbody.cpp", "sx_bdt.cpp"):
        assert len(re.findall(r"\bcollect\s*\(\s*\)", sources[name])) == 1, name


def test_reported_names_live_in_one_table():
    with open(os.path.join(CSRC, "sx_step_timer.hpp")) as f:
        timer = f.read()
    for table, names in (("kStageNames", STAGES), ("kKernelNames", KERNELS)):
        body = re.search(table + r"\[[^\]]*\]\s*=\s*\{([^}]*)\}", timer).group(1)
        assert re.findall(r'"([^"]+)"', body) == names
    for enum, names in (("Stage", STAGES), ("Kernel", KERNELS)):
        body = re.search(r"enum class " + enum + r"[^{]*\{([^}]*)\}", timer).group(1)
        assert [w.strip() for w in body.split(",")] == names + ["count"]
    # no second copy of a reported name as a string in the drivers
    for name, text in driver_sources().items():
        for s in re.findall(r'"([^"\n]+)"', text):
            assert s not in STAGES + KERNELS, "%s holds the reported name %r" % (name, s)
