"""A float64 forward-kinematics reference that shares no code with pytorch_volumetric_amd.kinematics or .transforms.

A robot is a literal table of rows
    (link, parent, joint type, axis, xyz, rpy, number of mesh visuals)
in declaration order.  Everything the tests expect of a robot -- its URDF text, the frame order, the joint columns, the leaf
slots, the pvamd_joint_t records and the frames themselves -- is derived here from that table alone, so that an error in
Chain.joint_table (joint columns, the parent remap, slot assignment), which the kernels and the CPU oracle would both
reproduce from the same bytes, does not reach the expected values.

Conventions (URDF): the frames are walked depth first, children in declaration order; the non-fixed joints take the columns of
q in that order; world[f] = world[parent] @ origin(xyz, rpy) @ motion(q); origin rotation = Rz(yaw) Ry(pitch) Rx(roll); a
revolute / continuous joint rotates about its normalised axis (Rodrigues), a prismatic joint translates along it.  Visual i of a
link sits at xyz = (0.01 (i + 1), 0, 0.01), rpy = (0, 0.1 (i + 1), 0) in the link frame: the visuals of one link differ.
"""
import numpy as np

FIXED, REVOLUTE, CONTINUOUS, PRISMATIC = "fixed", "revolute", "continuous", "prismatic"
JTYPE_CODE = {FIXED: 0, REVOLUTE: 1, CONTINUOUS: 1, PRISMATIC: 2}  # pvamd_joint_t.jtype

# 12 frames, 8 joints, 12 leaves: branching links (torso, shoulder, palm), links with 2 and 3 mesh visuals, mesh-less frames at
# the base, in the middle (lift) and at a tip (camera), fixed joints inside the tree, prismatic joints with skew axes
TREE = (
    ("base", None, None, None, None, None, 0),
    ("torso", "base", FIXED, None, (0, 0, 0.05), (0, 0, 0.3), 1),
    ("lift", "torso", PRISMATIC, (0, 0, 1), (0, 0, 0.2), (0.1, 0, 0), 0),
    ("shoulder", "lift", REVOLUTE, (0, 1, 0), (0.05, 0, 0.1), (0, 0.2, 0), 3),
    ("elbow", "shoulder", CONTINUOUS, (1, 1, 0), (0, 0, 0.25), (0.3, -0.2, 0.1), 1),
    ("palm", "elbow", REVOLUTE, (0, 0, -1), (0, 0, 0.2), (0, 0, 0), 2),
    ("finger_a", "palm", PRISMATIC, (0, 1, 0.5), (0, 0.03, 0.08), (0, 0, 0), 1),
    ("tip_a", "finger_a", FIXED, None, (0, 0, 0.05), (0, 0.4, 0), 1),
    ("finger_b", "palm", PRISMATIC, (0, -1, 0), (0, -0.03, 0.08), (0, 0, 0.2), 1),
    ("head", "torso", CONTINUOUS, (0, 0, 1), (0, 0, 0.6), (0, 0, 0), 1),
    ("camera", "head", FIXED, None, (0.05, 0, 0.05), (0, 0.3, 0), 0),
    ("antenna", "shoulder", REVOLUTE, (1, 0, 0), (0, 0.05, 0), (0, 0, 0), 1),
)

# fixed joints only: M == 0
STATIC = (
    ("pedestal", None, None, None, None, None, 1),
    ("column", "pedestal", FIXED, None, (0.02, -0.03, 0.3), (0.2, -0.1, 0.4), 0),
    ("plate", "column", FIXED, None, (0.1, 0.05, 0.15), (-0.3, 0.25, 0.1), 1),
)


def joint_name(link):
    return "j_" + link


def frames(table):
    """Rows of the table in frame order: depth first from the root, children in declaration order."""
    roots = [r for r in table if r[1] is None]
    assert len(roots) == 1
    out = []

    def visit(row):
        out.append(row)
        for child in table:
            if child[1] == row[0]:
                visit(child)

    visit(roots[0])
    assert len(out) == len(table)
    return out


def frame_names(table):
    return [r[0] for r in frames(table)]


def joint_names(table):
    """Names of the non-fixed joints in the order of their columns in q."""
    return [joint_name(r[0]) for r in frames(table) if r[1] is not None and r[2] != FIXED]


def prismatic_columns(table):
    moving = [r for r in frames(table) if r[1] is not None and r[2] != FIXED]
    return [c for c, r in enumerate(moving) if r[2] == PRISMATIC]


def leaf_links(table):
    """The link of every leaf: one leaf per mesh visual, in frame order."""
    return [r[0] for r in frames(table) for _ in range(r[6])]


def leaf_visuals(table):
    """(link, index of the visual within its link) of every leaf, in frame order."""
    return [(r[0], i) for r in frames(table) for i in range(r[6])]


def _fmt(v):
    return " ".join(repr(float(x)) for x in v)


def visual_xyz_rpy(i):
    assert 0 <= i < 9
    return (float(f"0.0{i + 1}"), 0.0, 0.01), (0.0, float(f"0.{i + 1}"), 0.0)  # the decimals the URDF text holds


def urdf(table, mesh_names):
    """URDF text of the table; mesh_names[s] = mesh file of leaf s (frame order)."""
    assert len(mesh_names) == len(leaf_links(table))
    parts = ['<robot name="fk_ref">']
    s = 0
    by_link = {}
    for row in frames(table):
        by_link[row[0]] = list(range(s, s + row[6]))
        s += row[6]
    for row in table:  # declaration order: the parser, not the file, has to find the frame order
        parts.append(f'<link name="{row[0]}">')
        for i, slot in enumerate(by_link[row[0]]):
            assert i < 9  # (visual_xyz_rpy reads the same decimals)
            parts.append(f'<visual><origin xyz="0.0{i + 1} 0 0.01" rpy="0 0.{i + 1} 0"/><geometry>'
                         f'<mesh filename="{mesh_names[slot]}"/></geometry></visual>')
        parts.append('</link>')
    for row in table:
        if row[1] is None:
            continue
        link, parent, jtype, axis, xyz, rpy, _ = row
        parts.append(f'<joint name="{joint_name(link)}" type="{jtype}"><parent link="{parent}"/><child link="{link}"/>'
                     f'<origin xyz="{_fmt(xyz)}" rpy="{_fmt(rpy)}"/>'
                     + ("" if axis is None else f'<axis xyz="{_fmt(axis)}"/>') + '</joint>')
    parts.append('</robot>')
    return "\n".join(parts)


def _rot(axis, angle):
    """Rodrigues' formula, (A,) angles about a unit axis -> (A, 3, 3) float64."""
    k = np.asarray(axis, dtype=np.float64)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    angle = np.asarray(angle, dtype=np.float64).reshape(-1, 1, 1)
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def origin64(xyz, rpy):
    m = np.eye(4)
    if xyz is None:
        return m
    r, p, y = (float(v) for v in rpy)
    m[:3, :3] = _rot((0, 0, 1), y)[0] @ _rot((0, 1, 0), p)[0] @ _rot((1, 0, 0), r)[0]
    m[:3, 3] = xyz
    return m


def fk64(table, q):
    """q: (A, M) joint values (any float dtype; taken as they are, in float64) -> (F, A, 4, 4) world_T_link, frame order."""
    fr = frames(table)
    q = np.asarray(q, dtype=np.float64)
    if q.ndim == 1:
        q = q[None]
    A = q.shape[0]
    index = {r[0]: i for i, r in enumerate(fr)}
    world = np.zeros((len(fr), A, 4, 4))
    col = 0
    for f, (link, parent, jtype, axis, xyz, rpy, _) in enumerate(fr):
        if parent is None:
            world[f] = np.eye(4)
            continue
        assert index[parent] < f
        motion = np.tile(np.eye(4), (A, 1, 1))
        if jtype != FIXED:
            k = np.asarray(axis, dtype=np.float64)
            k = k / np.linalg.norm(k)
            if jtype == PRISMATIC:
                motion[:, :3, 3] = q[:, col, None] * k
            else:
                motion[:, :3, :3] = _rot(k, q[:, col])
            col += 1
        world[f] = world[index[parent]] @ origin64(xyz, rpy) @ motion
    assert col == q.shape[1]
    return world


def visual_offsets64(table):
    """(S, 4, 4) link_T_visual of every leaf, frame order."""
    return np.stack([origin64(*visual_xyz_rpy(i)) for _, i in leaf_visuals(table)])


def _inv64(m):
    out = np.zeros_like(m)
    rt = np.swapaxes(m[..., :3, :3], -1, -2)
    out[..., :3, :3] = rt
    out[..., :3, 3] = -(rt @ m[..., :3, 3:4])[..., 0]
    out[..., 3, 3] = 1.0
    return out


def stack64(table, q, offsets, leaves=None):
    """offset[s]^-1 @ world[link(s)]^-1 as (S * A, 4, 4), leaf-major.  `leaves` = the link of every leaf (default: one per
    mesh visual in frame order); `offsets` (S, 4, 4) in the same order."""
    leaves = leaf_links(table) if leaves is None else list(leaves)
    names = frame_names(table)
    world = fk64(table, q)
    offsets = np.asarray(offsets, dtype=np.float64)
    assert offsets.shape == (len(leaves), 4, 4)
    out = [_inv64(offsets[s])[None] @ _inv64(world[names.index(link)]) for s, link in enumerate(leaves)]
    return np.concatenate(out)


def leaf_world64(table, q, leaves=None):
    """world[link(s)] as (S * A, 4, 4), leaf-major."""
    leaves = leaf_links(table) if leaves is None else list(leaves)
    names = frame_names(table)
    world = fk64(table, q)
    return np.concatenate([world[names.index(link)] for link in leaves])


def expected_records(table, leaves=None):
    """What Chain.joint_table(leaves) has to emit, from the table alone: a list of (parent, jtype, jcol, leaf_slot), one per
    pvamd_joint_t record.  Every frame gives one record; a link that fills several slots is followed by one fixed identity
    child per further slot.  parent = record index of the parent frame's own record; jcol counts the non-fixed joints."""
    leaves = leaf_links(table) if leaves is None else list(leaves)
    out, record_of, col = [], {}, 0
    for link, parent, jtype, *_ in frames(table):
        slots = [s for s, name in enumerate(leaves) if name == link]
        code = 0 if parent is None else JTYPE_CODE[jtype]
        me = record_of[link] = len(out)
        out.append((-1 if parent is None else record_of[parent], code, col if code else -1, slots[0] if slots else -1))
        col += 1 if code else 0
        for extra in slots[1:]:
            out.append((me, 0, -1, extra))
    return out


def frame_records(table, leaves=None):
    """The record index of every frame's own record (frame order), and {index of a duplicate record: link name}."""
    leaves = leaf_links(table) if leaves is None else list(leaves)
    own, dups, n = [], {}, 0
    for row in frames(table):
        own.append(n)
        extra = max(0, leaves.count(row[0]) - 1)
        for i in range(extra):
            dups[n + 1 + i] = row[0]
        n += 1 + extra
    return own, dups


def draw_q(table, A, scale, seed):
    """(A, M) float64 joint values: revolute / continuous columns randn * scale, prismatic columns uniform in +-0.3."""
    rng = np.random.default_rng(seed)
    M = len(joint_names(table))
    q = rng.standard_normal((A, M)) * scale
    for c in prismatic_columns(table):
        q[:, c] = rng.uniform(-0.3, 0.3, A)
    return q
