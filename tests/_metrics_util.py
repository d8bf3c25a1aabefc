"""Molecule pools shared by tests/test_metrics.py and tests/test_gpu_metrics.py.  A molecule is (types, edges): a list of
class ids and a list of (i, j, order)."""
import numpy as np


def pack(mols, n_max=None):
    """-> (orders int8 [B, n_max, n_max] strictly lower triangular, atom_type int32 [N], mol_off int32 [B+1])."""
    sizes = [len(t) for t, _ in mols]
    n_max = n_max or max(max(sizes, default=0), 1)
    orders = np.zeros((len(mols), n_max, n_max), np.int8)
    for b, (_, edges) in enumerate(mols):
        for i, j, o in edges:
            orders[b, max(i, j), min(i, j)] = o
    types = np.concatenate([np.asarray(t, np.int32) for t, _ in mols]) if mols else np.zeros(0, np.int32)
    return orders, types.astype(np.int32), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def renumber(mol, perm):
    """Atom a of `mol` becomes atom perm[a]."""
    types, edges = mol
    out = [0] * len(types)
    for a, t in enumerate(types):
        out[perm[a]] = t
    return out, [(perm[i], perm[j], o) for i, j, o in edges]


def random_pool(count=300, seed=0):
    """Molecule-like graphs: a random tree plus up to two ring closures, 3-9 atoms, 3 element types, orders 1-2."""
    rng = np.random.RandomState(seed)
    pool = []
    for _ in range(count):
        n = int(rng.randint(3, 10))
        edges = {(a, int(rng.randint(0, a))) for a in range(1, n)}
        for _ in range(int(rng.randint(0, 3))):
            i, j = (int(v) for v in rng.choice(n, 2, replace=False))
            edges.add((max(i, j), min(i, j)))
        pool.append(([int(t) for t in rng.randint(0, 3, n)], [(i, j, int(rng.randint(1, 3))) for i, j in sorted(edges)]))
    return pool


def atlas_set():
    """networkx's graph atlas: the connected graphs with 2-7 nodes and maximum degree <= 4, all carbon, single bonds.
    -> list of (molecule, independent cycles)."""
    import networkx as nx
    from networkx.generators.atlas import graph_atlas_g
    out = []
    for g in graph_atlas_g():
        n = g.number_of_nodes()
        if 2 <= n <= 7 and nx.is_connected(g) and max(d for _, d in g.degree()) <= 4:
            out.append((([0] * n, [(i, j, 1) for i, j in g.edges()]), g.number_of_edges() - n + 1))
    return out


def to_networkx(mol):
    import networkx as nx
    g = nx.Graph()
    for a, t in enumerate(mol[0]):
        g.add_node(a, t=t)
    for i, j, o in mol[1]:
        g.add_edge(i, j, o=o)
    return g


def chain(n, t=0, ring=False):
    return [t] * n, [(a, a - 1, 1) for a in range(1, n)] + ([(n - 1, 0, 1)] if ring else [])


# two fused six-rings (the ring 0..9 with the bridge 0-5) against two five-rings joined by a bond: same size, degrees
# and neighbour degrees, so plain colour refinement cannot tell them apart
DECALIN = ([0] * 10, [(a, a - 1, 1) for a in range(1, 10)] + [(9, 0, 1), (5, 0, 1)])
BICYCLOPENTYL = ([0] * 10, [(1, 0, 1), (2, 1, 1), (3, 2, 1), (4, 3, 1), (4, 0, 1),
                            (6, 5, 1), (7, 6, 1), (8, 7, 1), (9, 8, 1), (9, 5, 1), (5, 0, 1)])
