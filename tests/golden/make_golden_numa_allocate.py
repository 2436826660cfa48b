"""Writes tests/golden/numa_allocate_26.json — a hand transcription of the reference's
pkg/scheduler/plugins/nodenumaresource/resource_manager_test.go TestResourceManagerAllocate (:34-589), with source lines.

Every row runs on buildCPUTopologyForTest(2, 1, 26, 2) (:541): 104 cpus, NUMA node 0 = cpus 0-51, NUMA node 1 = 52-103
(it straddles cpu 64), two zones of 52 cpu / 128Gi (:542-557), node allocatable 104 cpu / 256Gi (:566-569), the
resource manager's strategy NUMALeastAllocated (:573).  A row gives Allocate its hint directly; through the plugin
surface the hint is what Filter stores, so a row is kept when a node NUMA policy (`numa_policy` below) and the row's
zone state make Filter store exactly the row's hint, and the tests check that stored mask before the allocation.  The
rows left out are listed with the reason.  `allocated` is the row's bound PodAllocation: its cpuset (cpus past 103 are
not in the topology) and per-NUMA cpu; with a ratio the zones' cpu is amplified (amplifyNUMANodeResources, :580).

Run: python tests/golden/make_golden_numa_allocate.py   (rewrites the JSON file next to this script)
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = "pkg/scheduler/plugins/nodenumaresource/resource_manager_test.go"


def rng(a, b):
    return list(range(a, b + 1))


ODD_HELD = [1, 3, 5] + rng(7, 103)  # cpuset "1,3,5,7-104"

CASES = [
    dict(line=93, name="allocate with required CPUBindPolicyFullPCPUs", cpus=4, required="FullPCPUs", hint=[0],
         numa_policy="SingleNUMANode", alloc=[], numa_allocated={}, ratio=0.0,
         want=rng(0, 3), want_numa={"0": "4"}),
    dict(line=124, name="allocate with required CPUBindPolicyFullPCPUs and allocated", cpus=4, required="FullPCPUs",
         hint=[0], numa_policy="SingleNUMANode", alloc=rng(4, 103), numa_allocated={"0": "48", "1": "52"}, ratio=0.0,
         want=rng(0, 3), want_numa={"0": "4"}),
    dict(line=216, name="allocate with required CPUBindPolicySpreadByPCPUs", cpus=4, required="SpreadByPCPUs", hint=[0],
         numa_policy="SingleNUMANode", alloc=[], numa_allocated={}, ratio=0.0,
         want=[0, 2, 4, 6], want_numa={"0": "4"}),
    dict(line=247, name="allocate with required CPUBindPolicySpreadByPCPUs and allocated", cpus=4,
         required="SpreadByPCPUs", hint=[0], numa_policy="SingleNUMANode", alloc=ODD_HELD,
         numa_allocated={"0": "48", "1": "52"}, ratio=0.0, want=[0, 2, 4, 6], want_numa={"0": "4"}),
    dict(line=339, name="allocate with required CPUBindPolicySpreadByPCPUs and amplified requests", cpus=4,
         required="SpreadByPCPUs", hint=[0], numa_policy="SingleNUMANode", alloc=[], numa_allocated={}, ratio=1.5,
         want=[0, 2, 4, 6], want_numa={"0": "4"}),
    dict(line=479, name="allocate by numa hint on mixed cpuset/share node", cpus=8, required="FullPCPUs", hint=[0, 1],
         numa_policy="BestEffort", alloc=rng(0, 43) + rng(53, 96), numa_allocated={"0": "48", "1": "48"}, ratio=0.0,
         want=rng(44, 47) + rng(98, 101), want_numa={"0": "4", "1": "4"}),
]

LEFT_OUT = [
    dict(line=45, name="allocate with non-existing resources in NUMA",
         reason="the row's point is a koordinator.sh/gpu-memory request that no zone reports; NodeNUMAResource's "
                "surface here carries cpu and memory only"),
    dict(line=74, name="allocate with insufficient resources",
         reason="54 cpu against the hint {0}: generateResourceHints never offers a 52-cpu NUMA node for 54 cpu, so no "
                "policy makes Filter store that hint"),
    dict(line=175, name="failed to allocate with required CPUBindPolicyFullPCPUs and allocated",
         reason="NUMA node 0 keeps cpus 0,2,4,6 but no whole core: trimNUMANodeResources leaves it 0 cpu, Filter "
                "offers no hint {0} and rejects the node before Allocate"),
    dict(line=298, name="failed to allocate with required CPUBindPolicySpreadByPCPUs and allocated",
         reason="cpus 0-3 are two cores: trimNUMANodeResources leaves NUMA node 0 2 cpu for 4, Filter offers no hint {0}"),
    dict(line=376, name="allocate with required CPUBindPolicySpreadByPCPUs and allocated and amplified requests",
         reason="the hint needs 6 amplified cpu on NUMA node 0, whose 4 free cpus trim to 4000m: Filter offers no hint "
                "{0}; the row passes only because Allocate is handed the hint"),
    dict(line=433, name="failed to allocate with CPU Share and allocated and amplified ratios",
         reason="NUMA node 0 has 3 amplified cpu left for 4: Filter offers no hint {0}"),
]


def main():
    for c in CASES + LEFT_OUT:
        c["source_line"] = f"{SRC}:{c['line']}"
    doc = {
        "source": f"{SRC} TestResourceManagerAllocate (:34-589)",
        "topo": [2, 1, 26, 2],
        "zones": [{"cpu": "52", "memory": "128Gi"}, {"cpu": "52", "memory": "128Gi"}],
        "node": {"cpu": "104", "memory": "256Gi"},
        "strategy": "LeastAllocated",
        "cases": CASES,
        "left_out": LEFT_OUT,
    }
    with open(os.path.join(HERE, "numa_allocate_26.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
