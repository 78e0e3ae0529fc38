"""One scene description, two builders.  Test infrastructure, like tests/scenes.py and tests/cameras.py.

`Desc` has hrt.Scene's constructor methods.  It records the calls and returns the ids the library returns, so a
builder written for hrt.Scene (tests/scenes.py) runs on it unchanged; `to_hrt` replays the record into an
hrt.Scene through the C ABI and `to_oracle` encodes it for the oracle's description entry point (oracle.cpp
build_desc), which assembles the same graph from the reference-shaped types.  The library's lowering and the
oracle's object graph then render one scene, and a test can hold the first to the second.

Ids: textures and materials are creation indices on both sides.  The library's node ids count every HNode it
pushes: a Cuboid's six sides come before it (hrt_node_cuboid) and a BvhNode of n objects pushes 2n - 1 nodes and
returns the last (scene.cpp build_bvh); `Desc` counts the same way, and `to_hrt` asserts every id the library
returns is the recorded one.  The oracle gives one id per node record, so `to_oracle` translates.

The description also carries the background and the camera spec in the tuple form of tests/cameras.py:
(look_from, look_at, fov, aperture, focus_dist, time0, time1).
"""
import copy

import numpy as np

import hrt
from oracle import oracle as O

MAGIC = 0x3144534F
# oracle.cpp D_*
OPS = {"solid": 1, "checker": 2, "noise": 3, "image": 4, "lambertian": 10, "metal": 11, "dielectric": 12,
       "diffuse_light": 13, "isotropic": 14, "sphere": 20, "moving_sphere": 21, "rect": 22, "cuboid": 23,
       "translate": 24, "rotate": 25, "constant_medium": 26, "list": 27, "bvh": 28}
NODE_OPS = ("sphere", "moving_sphere", "rect", "cuboid", "translate", "rotate", "constant_medium", "list", "bvh")
DEFAULT_CAMERA = ((13, 2, 3), (0, 0, 0), 20.0, 0.1, 10.0, 0.0, 1.0)  # tests/scenes.py camera()
DEFAULT_BACKGROUND = (0.7, 0.8, 1.0)  # hrt.params' default


def _f(*vals):
    return [float(np.float32(v)) for v in vals]


class Desc:
    def __init__(self, background=DEFAULT_BACKGROUND, camera=DEFAULT_CAMERA):
        self.calls = []  # (method name, args, the id returned)
        self.background = tuple(float(c) for c in background)
        self.camera = camera
        self.root = None
        self._n = {"tex": 0, "mat": 0, "node": 0}

    def copy(self):
        return copy.deepcopy(self)

    def _rec(self, cls, name, args, pushed=1):
        self._n[cls] += pushed
        rid = self._n[cls] - 1
        self.calls.append((name, args, rid))
        return rid

    # textures
    def solid(self, r, g, b):
        return self._rec("tex", "solid", _f(r, g, b))

    def checker(self, odd, even):
        return self._rec("tex", "checker", [int(odd), int(even)])

    def noise(self, scale, ranvec, perm):
        rv = np.array(ranvec, np.float32).reshape(-1)
        pm = np.array(perm, np.uint32).reshape(-1)
        assert rv.size == 768 and pm.size == 768
        return self._rec("tex", "noise", [float(np.float32(scale)), rv, pm])

    def image(self, data):
        return self._rec("tex", "image", [None if data is None else np.array(data, np.uint8)])

    # materials
    def lambertian(self, tex):
        return self._rec("mat", "lambertian", [int(tex)])

    def metal(self, albedo, fuzz):
        return self._rec("mat", "metal", [_f(*albedo), *_f(fuzz)])

    def dielectric(self, ior):
        return self._rec("mat", "dielectric", _f(ior))

    def diffuse_light(self, tex):
        return self._rec("mat", "diffuse_light", [int(tex)])

    def isotropic(self, tex):
        return self._rec("mat", "isotropic", [int(tex)])

    # hittables
    def sphere(self, center, radius, mat):
        return self._rec("node", "sphere", [_f(*center), *_f(radius), int(mat)])

    def moving_sphere(self, c0, c1, t0, t1, radius, mat):
        return self._rec("node", "moving_sphere", [_f(*c0), _f(*c1), *_f(t0, t1, radius), int(mat)])

    def rect(self, plane, a0, a1, b0, b1, k, mat):
        return self._rec("node", "rect", [int(plane), *_f(a0, a1, b0, b1, k), int(mat)])

    def cuboid(self, p0, p1, mat):
        return self._rec("node", "cuboid", [_f(*p0), _f(*p1), int(mat)], pushed=7)

    def translate(self, child, d):
        return self._rec("node", "translate", [int(child), _f(*d)])

    def rotate(self, axis, child, angle):
        return self._rec("node", "rotate", [int(axis), int(child), *_f(angle)])

    def constant_medium(self, boundary, density, tex):
        return self._rec("node", "constant_medium", [int(boundary), *_f(density), int(tex)])

    def list(self, children):
        return self._rec("node", "list", [[int(c) for c in children]])

    def bvh(self, children, t0=0.0, t1=1.0):
        ch = [int(c) for c in children]
        return self._rec("node", "bvh", [ch, *_f(t0, t1)], pushed=max(1, 2 * len(ch) - 1))

    def set_root(self, node):
        self.root = int(node)

    # the two builders
    def to_hrt(self, options=None) -> hrt.Scene:
        s = hrt.Scene()
        if options:
            s.set_options(**options)
        for name, args, rid in self.calls:
            got = getattr(s, name)(*args)
            assert got == rid, (name, got, rid)  # Desc counts ids as the library does
        s.set_root(self.root)
        return s

    def to_oracle(self) -> O.OracleScene:
        return O.OracleScene.from_description(*self.encode())

    def encode(self):
        """(u32 words, image byte blob) of oracle.cpp build_desc."""
        words, blob = [], bytearray()
        node_of = {}  # library node id -> the oracle's (one per node record)

        def u(*v):
            words.extend(np.array(v, np.uint32).reshape(-1).tolist())

        def f(*v):
            words.extend(np.array(v, np.float32).reshape(-1).view(np.uint32).tolist())

        lf, la, fov, ap, fd, t0, t1 = self.camera
        u(MAGIC, 0)
        f(*self.background, *lf, *la, fov, ap, fd, t0, t1)
        assert len(words) == 16
        for name, a, rid in self.calls:
            u(OPS[name])
            if name == "solid":
                f(*a)
            elif name == "checker":
                u(*a)
            elif name == "noise":
                f(a[0], *a[1])
                u(*a[2])
            elif name == "image":
                d = a[0]
                if d is None or d.size == 0:
                    u(0, 0, 0, 0)
                else:
                    h, w, c = d.shape
                    u(w, h, c, len(blob))
                    blob += d.tobytes()
            elif name in ("lambertian", "diffuse_light", "isotropic"):
                u(a[0])
            elif name == "metal":
                f(*a[0], a[1])
            elif name == "dielectric":
                f(a[0])
            elif name == "sphere":
                f(*a[0], a[1]); u(a[2])
            elif name == "moving_sphere":
                f(*a[0], *a[1], *a[2:5]); u(a[5])
            elif name == "rect":
                u(a[0]); f(*a[1:6]); u(a[6])
            elif name == "cuboid":
                f(*a[0], *a[1]); u(a[2])
            elif name == "translate":
                u(node_of[a[0]]); f(*a[1])
            elif name == "rotate":
                u(a[0], node_of[a[1]]); f(a[2])
            elif name == "constant_medium":
                u(node_of[a[0]]); f(a[1]); u(a[2])
            elif name == "list":
                u(len(a[0]), *[node_of[c] for c in a[0]])
            elif name == "bvh":
                f(a[1], a[2]); u(len(a[0]), *[node_of[c] for c in a[0]])
            if name in NODE_OPS:
                node_of[rid] = len(node_of)
        words[1] = node_of[self.root]
        return np.array(words, np.uint32), np.frombuffer(bytes(blob), np.uint8)

    # cameras and parameters of a render
    def spec(self, shutter=None):
        return self.camera if shutter is None else (*self.camera[:5], float(shutter[0]), float(shutter[1]))

    def hrt_camera(self, w, h, shutter=None):
        return hrt.camera(*self.spec(shutter), w, h)

    def params(self, w, h, spp, seed, depth=50, **kw):
        return hrt.params(w, h, spp, depth, seed, self.background, **kw)
