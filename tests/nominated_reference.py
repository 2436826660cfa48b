"""Plain model of nominated pods on top of the committed oracle (kg_nominated_pods_set,
kg_pods_schedule_staged_nominated, kg_pods_filter_nominated, the resident dry run): upstream's
RunFilterPluginsWithNominatedPods / addNominatedPods (k8s v1.24.15 framework/runtime/framework.go), restated as
published, in upstream's order of steps rather than the device's.

Per pod of the queue, in FIFO order:
  1. the oracle's keys on the plain node state: oracle.node_keys (NodeResourcesFit + LoadAware) and, with
     NodeNUMAResource, oracle.numa_eval per node (Filter, and its Score × weight added to the key's total);
  2. for each node holding applicable entries — live, priority >= the pod's, another uid — NodeInfo.AddPod of every
     such entry on a COPY of the node's state row (oracle.apply_pod: Requested of every resource, the pod count), then
     oracle.fit_filter on that copy and, with NodeNUMAResource, oracle.numa_eval with the copy's Requested cpu; the key
     is zeroed where either fails.  Scores stay the plain row's;
  3. the largest key wins, ties on the lowest node index;
  4. the pod is applied with oracle.apply_pod (with NodeNUMAResource: a one-node oracle.schedule_numa, which runs the
     plugin's Reserve on the oracle's NUMA state as well);
  5. the pod's own entry leaves the table when the pod was placed, whichever node it landed on."""
from dataclasses import dataclass

import numpy as np

from koordinator_amd import abi
from oracle import oracle

FIT_BITS = abi.REJECT_FIT_PODS | abi.REJECT_FIT_CPU | abi.REJECT_FIT_MEMORY | abi.REJECT_FIT_OTHER


@dataclass
class Entry:
    pod: np.ndarray   # one kg_pod record
    node: int
    priority: int
    live: bool = True

    @property
    def uid(self):
        return int(self.pod["uid"])


class Table:
    """the nominator: entries in the caller's order; stored() gives the engine's order, (node, priority descending),
    ties in the caller's order"""

    def __init__(self, pods=(), nodes=(), priorities=()):
        self.entries = [Entry(np.array(np.asarray(p, dtype=abi.POD_DTYPE).reshape(1)[0]), int(n), int(q))
                        for p, n, q in zip(pods, nodes, priorities)]

    def arrays(self):
        pods = (np.array([e.pod for e in self.entries], dtype=abi.POD_DTYPE) if self.entries
                else np.zeros(0, dtype=abi.POD_DTYPE))
        return (pods, np.array([e.node for e in self.entries], np.int32),
                np.array([e.priority for e in self.entries], np.int32))

    def applicable(self, node, priority, uid):
        return [e for e in self.entries if e.live and e.node == node and e.priority >= priority and e.uid != uid]

    def nodes_with_entries(self):
        return sorted({e.node for e in self.entries if e.live})

    def stored(self):
        """(uid, node, priority) of the live entries in stored order"""
        live = [e for e in self.entries if e.live]
        live.sort(key=lambda e: (e.node, -e.priority))  # stable
        return [(e.uid, e.node, e.priority) for e in live]

    def remove(self, uid):
        for e in self.entries:
            if e.live and e.uid == uid:
                e.live = False
                return True
        return False

    def pmax(self):
        return max((e.priority for e in self.entries if e.live), default=None)


def augmented_row(cfg, st, node, entries):
    """a copy of node's state row with every entry added as NodeInfo.AddPod does"""
    row = st[node:node + 1].copy()
    for e in entries:
        oracle.apply_pod(cfg, row, e.pod, 0)
    return row


def _numa_row(numa, i):
    return oracle.numa_state_export(numa["buf"], i, numa["rows"][i])


def augmented_reject(cfg, cluster, st, node, pod, entries, numa=None):
    """the KG_REJECT_FIT_* / KG_REJECT_NUMA bits of the pass on the row with `entries` added (0 = passes).  The oracle
    exposes NodeNUMAResource's Filter whole, so the NUMA bit is reported where the plain Filter passes and the augmented
    one does not; on a node the plain Filter already rejects, the scheduling result does not depend on it."""
    row = augmented_row(cfg, st, node, entries)
    rej = oracle.fit_filter(cluster.nodes[node:node + 1], row, pod) & FIT_BITS if cfg[0]["fit_filter"] else 0
    if numa is not None and cfg[0]["numa_filter"]:
        # only filterAmplifiedCPUs reads Requested; the rest of the plugin's Filter is the plain pass's business
        alloc = cluster.nodes[node]["allocatable"]
        plain_ok, _, _ = oracle.numa_eval(cfg, _numa_row(numa, node), pod,
                                          (int(st[node]["requested"][0]), int(st[node]["requested"][1])),
                                          (int(alloc[0]), int(alloc[1])))
        aug_ok, _, _ = oracle.numa_eval(cfg, _numa_row(numa, node), pod,
                                        (int(row[0]["requested"][0]), int(row[0]["requested"][1])),
                                        (int(alloc[0]), int(alloc[1])))
        if plain_ok and not aug_ok:
            rej |= abi.REJECT_NUMA
    return int(rej)


def plain_keys(cfg, cluster, st, pod, numa=None):
    keys = oracle.node_keys(cfg, cluster.nodes, cluster.metrics, st, pod, cluster.now_ns, 0, cluster.n)
    if numa is None:
        return keys
    w = int(cfg[0]["weight_numa"]) if cfg[0]["numa_score"] else 0
    for i in np.nonzero(keys)[0]:
        alloc = cluster.nodes[i]["allocatable"]
        ok, score, _ = oracle.numa_eval(cfg, _numa_row(numa, i), pod,
                                        (int(st[i]["requested"][0]), int(st[i]["requested"][1])),
                                        (int(alloc[0]), int(alloc[1])))
        if not ok:
            keys[i] = 0
        elif w:
            keys[i] = np.uint64(int(keys[i]) + ((score * w) << 32))
    return keys


def make_numa(node_numa):
    """the model's NodeNUMAResource state: the kg_node_numa rows and the oracle's per-node state buffer"""
    rows = np.ascontiguousarray(node_numa, dtype=abi.NODE_NUMA_DTYPE)
    return {"rows": rows, "buf": oracle.numa_states(rows), "size": int(oracle.lib().or_numa_state_size())}


def initial_states(cfg, cluster):
    st = oracle.states(cluster.n)
    if len(cluster.existing_pods):
        oracle.add_pods(cfg, st, cluster.existing_pods, cluster.existing_node)
    return st


def schedule(cfg, cluster, pods, priorities, table, numa=None, st=None):
    """FIFO scheduling of `pods` with the nominated pods of `table` honoured; mutates `table` (and `st` / `numa` when
    given).  Returns (node int32[n], total int64[n], st)."""
    pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
    st = initial_states(cfg, cluster) if st is None else st
    out_node = np.full(len(pods), -1, np.int32)
    out_score = np.zeros(len(pods), np.int64)
    for j in range(len(pods)):
        pod = pods[j:j + 1]
        uid, q = int(pod["uid"][0]), int(priorities[j])
        keys = plain_keys(cfg, cluster, st, pod, numa)
        for i in table.nodes_with_entries():
            if keys[i] == 0:
                continue
            add = table.applicable(i, q, uid)
            if add and augmented_reject(cfg, cluster, st, i, pod, add, numa) != 0:
                keys[i] = 0
        best = int(keys.max()) if len(keys) else 0
        if best == 0:
            continue
        w = 0xFFFFFFFF - (best & 0xFFFFFFFF)
        if numa is None:
            oracle.apply_pod(cfg, st, pod, w)
        else:  # Reserve on the winner alone: NodeInfo, the assign cache and the NUMA state of that node
            sz = numa["size"]
            got, _ = oracle.schedule_numa(cfg, cluster.nodes[w:w + 1], cluster.metrics[w:w + 1], st[w:w + 1],
                                          numa["buf"][w * sz:(w + 1) * sz], pod, cluster.now_ns)
            if got[0] < 0:  # the cpuset allocation failed at Reserve: the pod stays unplaced
                continue
        out_node[j], out_score[j] = w, best >> 32
        table.remove(uid)
    return out_node, out_score, st


def filter_nominated(cfg, cluster, st, pod, priority, table, numa=None):
    """kg_pods_filter_nominated: per node (reject bits of the augmented pass, entries added)"""
    pod = np.ascontiguousarray(np.asarray(pod, dtype=abi.POD_DTYPE).reshape(1))
    rej, added = np.zeros(cluster.n, np.int32), np.zeros(cluster.n, np.int32)
    for i in range(cluster.n):
        add = table.applicable(i, int(priority), int(pod["uid"][0]))
        added[i] = len(add)
        rej[i] = augmented_reject(cfg, cluster, st, i, pod, add, numa)
    return rej, added


def select_victims(cfg, cluster, st, node, pod, priority, table, victims, violating, numa=None):
    """the dry run of one candidate with the nominated pods added: oracle.select_victims on the augmented state row
    (the entries stay added while the victims are removed and reprieved)"""
    pod = np.ascontiguousarray(np.asarray(pod, dtype=abi.POD_DTYPE).reshape(1))
    add = table.applicable(node, int(priority), int(pod["uid"][0]))
    row = augmented_row(cfg, st, node, add)
    return oracle.select_victims(cfg, cluster.nodes[node], cluster.metrics[node], row, None, pod, victims, None,
                                 violating, cluster.now_ns,
                                 numa=None if numa is None else _numa_row(numa, node))
