"""CPU: the Makefile's printed object list (make print-objects) is THE list of libnpb.so's translation units -- every source of csrc/
is in it, and the tools that link a variant of the library take their link lists from it.  No build, no GPU."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nuclear_sim_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_every_source_is_linked_and_the_mutation_tools_link_by_the_same_list():
    import mutate_device
    import scattered_calls_mutants
    objects = subprocess.run(["make", "-s", "-C", CSRC, "print-objects"], check=True, capture_output=True, text=True).stdout.split()
    assert len(objects) == len(set(objects))
    # every *.hip and *.cpp of csrc/ is an object of the list, and the list names nothing else
    sources = sorted(os.path.splitext(f)[0] for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp")))
    assert sorted(set(re.sub(r"(_f64|_f32)?\.o$", "", o) for o in objects)) == sources
    # a unit built for fp32 storage is built for fp64 storage too
    assert all(o.replace("_f32.o", "_f64.o") in objects for o in objects if o.endswith("_f32.o"))
    # the mutation tools recompile one object and link every other one of the list: one function, no list of their own
    build = os.path.join(ROOT, "nuclear_sim_amd", "build")
    assert mutate_device.MUTATED in objects
    assert mutate_device.link_objects() == [os.path.join(build, o) for o in objects if o != mutate_device.MUTATED]
    assert scattered_calls_mutants.link_objects is mutate_device.link_objects
    for tool in ("mutate_device.py", "scattered_calls_mutants.py"):
        text = open(os.path.join(ROOT, "tools", tool)).read()
        assert "link_objects()" in text
        named = set(re.findall(r"\bnp\w+\.o\b", text))
        assert named <= {mutate_device.MUTATED}, "%s names objects of its own: %s" % (tool, sorted(named))
