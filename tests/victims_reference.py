"""Reference for the resident bound-pod table (kg_node_bound_pods_set, kg_pods_select_victims_resident,
kg_pods_preempt_resident): what a caller builds per node today before kg_pods_select_victims — the front half of
SelectVictimsOnNode, restated as published, in upstream's order of steps rather than the device's:

  1. walk NodeInfo.Pods in the caller's order and keep the pods canPreempt accepts
     (koordinator elasticquota/preempt.go:139-147, 283-294; upstream's defaultpreemption keeps every pod of lower priority);
  2. sort them with util.MoreImportantPod (k8s.io/kubernetes pkg/scheduler/util): higher priority first, then the
     earlier start.  Upstream's sort.Slice is unstable; the project's rule is that ties keep the caller's order;
  3. filterPodsWithPDBViolation (preempt.go:222-267): a fresh copy of the budgets, every pod decrements every PDB it
     matches, and it is violating when one of them drops below zero;
  4. the reprieve order: the violating pods, then the others."""
from dataclasses import dataclass, field


def can_preempt(pod_priority, pod_quota, vic_priority, vic_quota, vic_non_preemptible, quota_rule):
    if not quota_rule:
        return pod_priority > vic_priority
    if vic_non_preemptible:
        return False
    return pod_priority > vic_priority and pod_quota == vic_quota


def more_important_order(indices, priority, start):
    """the indices sorted by MoreImportantPod; Python's sort is stable"""
    return sorted(indices, key=lambda k: (-int(priority[k]), int(start[k])))


def filter_pods_with_pdb_violation(pods, mask, pdb_allowed):
    """(violating, non-violating) of `pods` (indices, in order); mask[k] bit b = pod k matches PDB b"""
    allowed = [int(a) for a in pdb_allowed]
    violating, others = [], []
    for k in pods:
        violated = False
        for b in range(len(allowed)):
            if not (int(mask[k]) >> b) & 1:
                continue
            allowed[b] -= 1
            if allowed[b] < 0:
                violated = True
        (violating if violated else others).append(k)
    return violating, others


@dataclass
class NodeVictims:
    stored: list = field(default_factory=list)      # every pod of the node, caller indices in MoreImportantPod order
    order: list = field(default_factory=list)       # the potential victims, caller indices in reprieve order
    violating: list = field(default_factory=list)   # per entry of `order`: PDB-violating
    reordered: bool = False                         # the PDB split changed the sorted order


def node_victims(pod_priority, pod_quota, quota_rule, priority, start, quota, non_preemptible, mask, pdb_allowed):
    """one node's list (arrays in the caller's order) → NodeVictims"""
    n = len(priority)
    potential = [k for k in range(n)
                 if can_preempt(pod_priority, pod_quota, int(priority[k]), int(quota[k]), bool(non_preemptible[k]), quota_rule)]
    ranked = more_important_order(potential, priority, start)
    vio, others = filter_pods_with_pdb_violation(ranked, mask, pdb_allowed)
    return NodeVictims(stored=more_important_order(range(n), priority, start), order=vio + others,
                       violating=[True] * len(vio) + [False] * len(others), reordered=(vio + others) != ranked)
