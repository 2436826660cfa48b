"""Reference for kg_pods_pick_candidate / kg_pods_preempt: upstream's SelectCandidate → pickOneNodeForPreemption
(k8s.io/kubernetes v1.24 pkg/scheduler/framework/preemption/preemption.go) and GetEarliestPodStartTime
(pkg/scheduler/util), restated as published: successive narrowing passes over a list of candidates, each keeping the
candidates that tie on the pass's minimum — not the device's formulation (one wide key, one minimum).

Upstream iterates a Go map where this walks the candidates in call order; what still ties at the end goes to the lowest
position (the project's rule).  `rule` reports which step left exactly one candidate: 0 = a candidate without victims,
1 = PDB violations, 2 = the first victim's priority, 3 = the priority sum, 4 = the victim count, 5 = the latest earliest
start, 6 = the position; None = no eligible candidate."""
from dataclasses import dataclass, field

MAX_INT32 = 2**31 - 1
MAX_INT64 = 2**63 - 1


@dataclass
class Candidate:
    position: int
    node: int
    pods: list            # positions k into the victims array, in list order (Victims.Pods)
    num_pdb_violations: int


@dataclass
class Pick:
    candidate: int = -1
    node_idx: int = -1
    eligible: int = 0
    n_victims: int = 0
    num_violating: int = 0
    first_priority: int = 0
    sum_priorities: int = 0
    earliest_start_unix_nano: int = 0
    victims: list = field(default_factory=list)
    rule: int | None = None

    def record(self):
        """the fields of abi.PREEMPT_PICK_DTYPE, in order"""
        return (self.candidate, self.node_idx, self.eligible, self.n_victims, self.num_violating, self.first_priority,
                self.sum_priorities, self.earliest_start_unix_nano)


def earliest_pod_start_time(pods, priority, start):
    """util.GetEarliestPodStartTime: the earliest start among the pods holding the highest priority, found in one walk
    with a running maximum.  None without pods."""
    if not pods:
        return None
    earliest = int(start[pods[0]])
    max_priority = int(priority[pods[0]])
    for k in pods:
        p = int(priority[k])
        if p == max_priority:
            if int(start[k]) < earliest:
                earliest = int(start[k])
        elif p > max_priority:
            max_priority = p
            earliest = int(start[k])
    return earliest


def sum_priorities(pods, priority):
    total = 0
    for k in pods:
        # "We add MaxInt32+1 to all priorities to make all of them >= 0."
        total += int(priority[k]) + (MAX_INT32 + 1)
    return total


def pick_one_node(cands, priority, start):
    """pickOneNodeForPreemption over a non-empty candidate list → (Candidate, rule)"""
    for c in cands:
        if len(c.pods) == 0:
            return c, 0  # "We found a node that doesn't need any preemption. Return it!"
    # 1. minimum number of PDB violations
    min_violating = MAX_INT32
    nodes1 = []
    for c in cands:
        if c.num_pdb_violations < min_violating:
            min_violating = c.num_pdb_violations
            nodes1 = []
        if c.num_pdb_violations == min_violating:
            nodes1.append(c)
    if len(nodes1) == 1:
        return nodes1[0], 1
    # 2. minimum highest-priority victim, which upstream reads from victims.Pods[0]
    min_highest = MAX_INT32
    nodes2 = []
    for c in nodes1:
        highest = int(priority[c.pods[0]])
        if highest < min_highest:
            min_highest = highest
            nodes2 = []
        if highest == min_highest:
            nodes2.append(c)
    if len(nodes2) == 1:
        return nodes2[0], 2
    # 3. minimum sum of priorities
    min_sum = MAX_INT64
    nodes1 = []
    for c in nodes2:
        s = sum_priorities(c.pods, priority)
        if s < min_sum:
            min_sum = s
            nodes1 = []
        if s == min_sum:
            nodes1.append(c)
    if len(nodes1) == 1:
        return nodes1[0], 3
    # 4. minimum number of pods
    min_pods = MAX_INT32
    nodes2 = []
    for c in nodes1:
        if len(c.pods) < min_pods:
            min_pods = len(c.pods)
            nodes2 = []
        if len(c.pods) == min_pods:
            nodes2.append(c)
    if len(nodes2) == 1:
        return nodes2[0], 4
    # 5. the latest earliest start time; a strict After, so the first of equals stays
    latest = earliest_pod_start_time(nodes2[0].pods, priority, start)
    chosen = nodes2[0]
    for c in nodes2[1:]:
        t = earliest_pod_start_time(c.pods, priority, start)
        if t > latest:
            latest = t
            chosen = c
    tied = [c for c in nodes2 if earliest_pod_start_time(c.pods, priority, start) == latest]
    return chosen, 5 if len(tied) == 1 else 6


def pick_candidate(nodes, offsets, reject, kept, num_violating, priority, start) -> Pick:
    """The pick over the arrays kg_pods_pick_candidate takes."""
    cands = []
    for c in range(len(nodes)):
        if int(reject[c]) != 0:
            continue
        pods = [k for k in range(int(offsets[c]), int(offsets[c + 1])) if kept[k]]
        cands.append(Candidate(c, int(nodes[c]), pods, int(num_violating[c])))
    out = Pick(eligible=len(cands))
    if not cands:
        return out
    w, rule = pick_one_node(cands, priority, start)
    out.candidate, out.node_idx, out.rule, out.victims = w.position, w.node, rule, list(w.pods)
    out.n_victims = len(w.pods)
    if w.pods:
        out.num_violating = w.num_pdb_violations
        out.first_priority = int(priority[w.pods[0]])
        out.sum_priorities = sum_priorities(w.pods, priority)
        out.earliest_start_unix_nano = earliest_pod_start_time(w.pods, priority, start)
    return out
