"""Pose evaluation for skinned meshes, on the host in binary64: a glTF animation sampled at a time, the node tree composed, and the
joint palette nxhip_pose_blas takes (include/nexus_hip.h).  The cost is per joint, not per vertex; the vertices are blended on the
device (nexus_amd/csrc/device/nx_skin.hip).  Reads what loaders.load_glb(skins=True) fills: LoadedScene.nodes, skins, animations.
The C++ twin is nexus::Scene::JointPalette."""
import numpy as np

NLERP_BELOW = 1e-9  # 1 - |q0 . q1| under this: the arc is too short for sin(theta) to divide by; normalised lerp instead


def _quat_matrix(q):
    """rotation matrix of a quaternion (x, y, z, w), normalised first"""
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def slerp(q0, q1, u):
    """shortest-arc spherical interpolation of two unit quaternions"""
    q0, q1 = np.asarray(q0, np.float64), np.asarray(q1, np.float64)
    d = float(np.dot(q0, q1))
    if d < 0.0:
        q1, d = -q1, -d
    if 1.0 - d < NLERP_BELOW:
        q = (1.0 - u) * q0 + u * q1
    else:
        theta = np.arccos(min(d, 1.0))
        q = (np.sin((1.0 - u) * theta) * q0 + np.sin(u * theta) * q1) / np.sin(theta)
    return q / np.linalg.norm(q)


def sample_channel(channel, t):
    """the channel's value at time t, clamped to its first and last key"""
    times, values = channel["times"], channel["values"]
    if t <= times[0]:
        return np.array(values[0], np.float64)
    if t >= times[-1]:
        return np.array(values[-1], np.float64)
    i = int(np.searchsorted(times, t, side="right")) - 1  # times[i] <= t < times[i + 1]
    if channel["interpolation"] == "STEP":
        return np.array(values[i], np.float64)
    u = (t - times[i]) / (times[i + 1] - times[i])
    if channel["path"] == "rotation":
        return slerp(values[i], values[i + 1], u)
    return (1.0 - u) * np.asarray(values[i], np.float64) + u * np.asarray(values[i + 1], np.float64)


def node_world_matrices(scene, animation=None, t=0.0):
    """the 4 x 4 world matrix of every node of scene.nodes with `animation` (an index into scene.animations, one of its entries, or
    None: the rest pose) sampled at t"""
    if animation is not None and not isinstance(animation, dict):
        animation = scene.animations[int(animation)]
    trs = [dict(translation=n["translation"], rotation=n["rotation"], scale=n["scale"]) for n in scene.nodes]
    animated = set()
    for ch in (animation["channels"] if animation is not None else []):
        if ch["path"] == "weights":
            continue  # (morph_weights)
        trs[ch["node"]][ch["path"]] = sample_channel(ch, float(t))
        animated.add(ch["node"])
    world = [None] * len(scene.nodes)

    def local(i):
        n = scene.nodes[i]
        if n["matrix"] is not None and i not in animated:
            return n["matrix"]
        m = np.eye(4)
        m[:3, :3] = _quat_matrix(np.asarray(trs[i]["rotation"], np.float64)) * np.asarray(trs[i]["scale"], np.float64)[None, :]
        m[:3, 3] = trs[i]["translation"]
        return m

    def resolve(i):
        if world[i] is None:
            p = scene.nodes[i]["parent"]
            world[i] = local(i) if p < 0 else resolve(p) @ local(i)
        return world[i]

    for i in range(len(scene.nodes)):
        resolve(i)
    return world


def joint_palette(scene, skin, animation=None, t=0.0):
    """(jointCount, 12) float32 for Context.pose_blas: row j = the 3 x 4 object-space matrix
    inverse(meshNodeWorld) x jointWorld[j] x inverseBind[j] (glTF's formula; the instance's own matrix puts meshNodeWorld back), evaluated
    in binary64 and rounded once.  skin: an index into scene.skins or one of its entries; animation: likewise, None = the rest pose."""
    if not isinstance(skin, dict):
        skin = scene.skins[int(skin)]
    world = node_world_matrices(scene, animation, t)
    to_mesh = np.linalg.inv(world[skin["mesh_node"]])
    rows = [(to_mesh @ world[j] @ skin["inverse_bind"][k])[:3, :].reshape(12) for k, j in enumerate(skin["joints"])]
    return np.array(rows, np.float64).astype(np.float32)


def morph_weights(scene, morph, animation=None, t=0.0):
    """(targets,) float32 for Context.pose_blas_morph: the morph's default weights, or — where `animation` has a `weights` channel on the node
    that places the mesh — that channel at t by sample_channel's rule, evaluated in binary64 and rounded once.  morph: an index into
    scene.morphs or one of its entries; animation: an index into scene.animations, one of its entries, or None = the defaults."""
    if not isinstance(morph, dict):
        morph = scene.morphs[int(morph)]
    if animation is not None and not isinstance(animation, dict):
        animation = scene.animations[int(animation)]
    for ch in (animation["channels"] if animation is not None else []):
        if ch["path"] == "weights" and ch["node"] == morph["mesh_node"]:
            w = sample_channel(ch, float(t))
            if len(w) != len(morph["weights"]):
                raise ValueError("the weights channel has %d values per key and the mesh %d targets" % (len(w), len(morph["weights"])))
            return np.asarray(w, np.float64).astype(np.float32)
    return np.array(morph["weights"], np.float32)
