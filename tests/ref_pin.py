"""The reference pin's shared code: the scene / result file formats of oracle/ref_pin/*.cpp and
the one call plan that the pin drivers, the oracle and the GPU engine all run.

Scene file of ref_pin_core (little-endian, no padding): "DMFPIN01", int32 H, W, float32 K[9],
float64 bounds[6], int32 mode (0 setVolumeSize, 1 setResolution), int32 dims[3], float64
res[3], int32 flags (bit 0: also the no-normals integratePointCloud; bit 1: also the functions
that index voxels_ unguarded), int32 n, float32 xyz[3n], float32 normals[3n], int32 P, float32
poses[12P], then the probes: int32 n, int32 (r, c, depth)[n] | int32 n, float64 xyz[3n], int32
pose[n] | int32 n, float64 xyz[3n] | int32 n, int32 (r, c)[n] | int32 n, float64 radians[n] |
int32 n, float32 xyz[3n] (validPoints / getVoxel).
Scene file of ref_pin_ogrid: "DMFPIN02", float64 bounds[6], float32 res[3], int32 k, int32 n,
float32 cloud[3n], int32 m, float32 normals[6m], int32 n_first.
Result file: records of uint32 name length, name, uint32 type code, uint64 byte count, data.

A fixture tests/golden/ref_pin_<scene>.npz holds the scene as in_* / og_in_* arrays, every
record of the reference's result files as out_* arrays, and a JSON `meta`.
"""
import json
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF_BIN = os.path.join(ROOT, "oracle", "_ref")
REFERENCE = os.environ.get("DMF_REFERENCE", "/root/reference")
SCENES = ("exact", "general", "general_trunc", "one", "empty")
CODES = {0: np.uint8, 1: np.int32, 2: np.int64, 3: np.uint64, 4: np.float32, 5: np.float64}
CORE_IN = ("H", "W", "K", "bounds", "mode", "dims", "res", "flags", "xyz", "nrm", "poses", "proj", "tr", "tr_pose",
           "dep", "vp", "deg", "vpt")
OG_IN = ("bounds", "res", "k", "cloud", "nrm", "n_first")


def fixture_path(scene):
    return os.path.join(GOLDEN, f"ref_pin_{scene}.npz")


def load(scene):
    z = np.load(fixture_path(scene))
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    return d


def has_ogrid(fx):
    return "og_in_cloud" in fx


def expected(fx, prefix="out_"):
    return {k[len(prefix):]: v for k, v in fx.items() if k.startswith(prefix)}


# ------------------------------------------------------------------------------ files
def _a(x, dt):
    return np.ascontiguousarray(x, dt).tobytes()


def core_scene_bytes(fx):
    g = lambda k: fx["in_" + k]
    n, P = g("xyz").reshape(-1, 3).shape[0], g("poses").reshape(-1, 12).shape[0]
    b = [b"DMFPIN01", struct.pack("<ii", int(g("H")), int(g("W"))), _a(g("K"), "<f4"), _a(g("bounds"), "<f8"),
         struct.pack("<i", int(g("mode"))), _a(g("dims"), "<i4"), _a(g("res"), "<f8"),
         struct.pack("<i", int(g("flags"))), struct.pack("<i", n), _a(g("xyz"), "<f4"), _a(g("nrm"), "<f4"),
         struct.pack("<i", P), _a(g("poses"), "<f4")]
    b += [struct.pack("<i", g("proj").reshape(-1, 3).shape[0]), _a(g("proj"), "<i4")]
    b += [struct.pack("<i", g("tr").reshape(-1, 3).shape[0]), _a(g("tr"), "<f8"), _a(g("tr_pose"), "<i4")]
    b += [struct.pack("<i", g("dep").reshape(-1, 3).shape[0]), _a(g("dep"), "<f8")]
    b += [struct.pack("<i", g("vp").reshape(-1, 2).shape[0]), _a(g("vp"), "<i4")]
    b += [struct.pack("<i", g("deg").size), _a(g("deg"), "<f8")]
    b += [struct.pack("<i", g("vpt").reshape(-1, 3).shape[0]), _a(g("vpt"), "<f4")]
    return b"".join(b)


def ogrid_scene_bytes(fx):
    g = lambda k: fx["og_in_" + k]
    return b"".join([b"DMFPIN02", _a(g("bounds"), "<f8"), _a(g("res"), "<f4"), struct.pack("<i", int(g("k"))),
                     struct.pack("<i", g("cloud").reshape(-1, 3).shape[0]), _a(g("cloud"), "<f4"),
                     struct.pack("<i", g("nrm").reshape(-1, 6).shape[0]), _a(g("nrm"), "<f4"),
                     struct.pack("<i", int(g("n_first")))])


def parse_result(raw):
    out, o = {}, 0
    while o < len(raw):
        (ln,) = struct.unpack_from("<I", raw, o)
        name = raw[o + 4:o + 4 + ln].decode()
        code, nbytes = struct.unpack_from("<IQ", raw, o + 4 + ln)
        o += 16 + ln
        out[name] = np.frombuffer(raw[o:o + nbytes], np.dtype(CODES[code]).newbyteorder("<")).copy()
        o += nbytes
    assert o == len(raw)
    return out


def start_binary(exe, scene_bytes, tmp, tag):
    """Starts exe on a scene; returns a function that waits and gives the raw result file."""
    sp, rp = os.path.join(tmp, tag + ".scene"), os.path.join(tmp, tag + ".result")
    with open(sp, "wb") as f:
        f.write(scene_bytes)
    p = subprocess.Popen([exe, sp, rp], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)

    def finish():
        err = p.communicate(timeout=900)[1]
        assert p.returncode == 0, (exe, p.returncode, err[-2000:])
        with open(rp, "rb") as f:
            return f.read()
    return finish


# ------------------------------------------------------------------------------ the plan
class OracleBackend:
    """oracle/oracle.py behind the names the plan uses."""

    def __init__(self, O):
        self.O = O

    def volume(self):
        return self.O.Volume()

    def engine(self, K, H, W):
        return self.O.Engine(K, H, W)

    def info(self, v):
        i = v.info()
        return ([i["xdim_"], i["ydim_"], i["zdim_"]], [i["xdelta_"], i["ydelta_"], i["zdelta_"], i["voxel_size_"]],
                i["hsize_"])

    def flags(self, v):
        return v.voxel_table()[:2]

    def counts(self, v):
        return v.voxel_table()[2:]

    def probes(self, fx):
        O, g = self.O, (lambda k: fx["in_" + k])
        K, poses = g("K"), g("poses").reshape(-1, 12)
        return {"probe_project": [O.project_point(K, *map(int, q)) for q in g("proj").reshape(-1, 3)],
                "probe_transform": [O.transform_point(poses[p], *q) for q, p in zip(g("tr").reshape(-1, 3), g("tr_pose"))],
                "probe_deproject": [O.deproject_point(K, *q) for q in g("dep").reshape(-1, 3)],
                "probe_validpixel": [O.valid_pixel(int(g("H")), int(g("W")), *map(int, q)) for q in g("vp").reshape(-1, 2)],
                "probe_degree": [O.degree(r) for r in g("deg")]}

    def ogrid(self):
        return self.O.OccupancyGrid()

    def ogrid_downloads(self, G):
        return G.download(0), G.download(1), G.downloadReorganizedCloud(False), G.downloadReorganizedCloud(True)


class GpuBackend:
    """dmf_amd (libdmf.so) behind the names the plan uses.  `integrate` replaces the host
    integratePointCloud (the device entry point); `setup` is called on every new volume (knobs)."""

    def __init__(self, dmf, integrate=None, setup=None):
        self.dmf, self.integrate, self.setup = dmf, integrate, setup

    def volume(self):
        v = self.dmf.VoxelVolume()
        if self.integrate:
            v.integratePointCloud = lambda xyz, nrm=None: self.integrate(v, xyz, nrm)
        return v

    def engine(self, K, H, W):
        return self.dmf.RayTracingEngine(self.dmf.Camera(K, H, W))

    def info(self, v):
        i = v.info()
        return ([i["xdim"], i["ydim"], i["zdim"]], [i["xdelta"], i["ydelta"], i["zdelta"], i["voxel_size"]],
                i["hsize"])

    def flags(self, v):
        return v.voxel_flags()

    def counts(self, v):
        return v.voxel_counts()

    def probes(self, fx):
        g = lambda k: fx["in_" + k]
        cam, poses = self.dmf.Camera(g("K"), int(g("H")), int(g("W"))), g("poses").reshape(-1, 12)
        return {"probe_project": [cam.projectPoint(*map(int, q)) for q in g("proj").reshape(-1, 3)],
                "probe_transform": [cam.transformPoints(*q, poses[p]) for q, p in zip(g("tr").reshape(-1, 3), g("tr_pose"))],
                "probe_deproject": [cam.deProjectPoint(*q) for q in g("dep").reshape(-1, 3)],
                "probe_validpixel": [cam.validPixel(*map(int, q)) for q in g("vp").reshape(-1, 2)],
                "probe_degree": [self.dmf.degree(r) for r in g("deg")]}

    def ogrid(self):
        return self.dmf.OccupancyGrid()

    def ogrid_downloads(self, G):
        return G.downloadCloud(), G.downloadHQCloud(), G.downloadReorganizedCloud(False), G.downloadReorganizedCloud(True)


PROBE_TYPES = {"probe_project": np.float32, "probe_transform": np.float32, "probe_deproject": np.int32,
               "probe_validpixel": np.uint8, "probe_degree": np.int32}


def make_volume(B, fx, normals=True):
    g = lambda k: fx["in_" + k]
    v = B.volume()
    v.setDimensions(*map(float, g("bounds")))
    if int(g("mode")) == 0:
        v.setVolumeSize(*map(int, g("dims")))
    else:
        v.setResolution(*map(float, g("res")))
    v.constructVolume()
    if getattr(B, "setup", None):
        B.setup(v)
    v.integratePointCloud(g("xyz").reshape(-1, 3), g("nrm").reshape(-1, 3) if normals else None)
    return v


class _Calls:
    def __init__(self, B):
        self.B, self.c = B, {k: [] for k in ("found", "ret", "count", "list", "view", "good")}

    def add(self, v, found=False, ret=0, lst=None):
        c = self.c
        c["found"].append(int(bool(found)))
        c["ret"].append(int(ret))
        c["count"].append(0 if lst is None else len(lst))
        c["list"].append(np.zeros(0, np.uint64) if lst is None else np.asarray(lst, np.uint64))
        view, good = self.B.flags(v)
        c["view"].append(np.asarray(view, np.int32))
        c["good"].append(np.asarray(good, np.uint8))

    def out(self, pre):
        c = self.c
        cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
        return {pre + "_found": np.array(c["found"], np.uint8), pre + "_ret": np.array(c["ret"], np.int32),
                pre + "_count": np.array(c["count"], np.int64), pre + "_list": cat(c["list"], np.uint64),
                pre + "_view": cat(c["view"], np.int32), pre + "_good": cat(c["good"], np.uint8)}


def run_volume(B, fx):
    """The volume records (ref_pin_core.cpp's first part)."""
    out = {}
    v = make_volume(B, fx, True)
    dims, deltas, hsize = B.info(v)
    out["vol_dims"] = np.array(dims, np.int32)
    out["vol_deltas"] = np.array(deltas, np.float64)
    out["vol_hsize"] = np.array([hsize], np.uint64)
    out["occ"] = np.asarray(v.occupied_cells_, np.uint64)
    npts, nnrm = B.counts(v)
    out["occ_npts"], out["occ_nnrm"] = np.asarray(npts, np.int32), np.asarray(nnrm, np.int32)
    if int(fx["in_flags"]) & 1:
        v = make_volume(B, fx, False)
        out["nn_occ"] = np.asarray(v.occupied_cells_, np.uint64)
        npts, nnrm = B.counts(v)
        out["nn_npts"], out["nn_nnrm"] = np.asarray(npts, np.int32), np.asarray(nnrm, np.int32)
    return out


def run_camera_probes(B, fx):
    """Camera's helpers and degree(): host formulas on every side, no volume needed."""
    return {k: np.array(v, PROBE_TYPES[k]).reshape(-1) for k, v in B.probes(fx).items()}


def run_volume_probes(B, fx, v=None):
    """validPoints and getVoxel of the scene's volume."""
    v, pts = v or make_volume(B, fx), fx["in_vpt"].reshape(-1, 3)
    return {"probe_validpoints": np.array([v.validPoints(*p) for p in pts], np.uint8),
            "probe_getvoxel": np.array([v.getVoxel(*p) for p in pts], np.int32).reshape(-1)}


def run_probes(B, fx):
    return {**run_camera_probes(B, fx), **run_volume_probes(B, fx)}


FWD_FUNCTIONS = ("rayTrace", "rayTraceAndClassify", "rayTraceAndGetGoodPoints", "rayTraceAndGetPoints",
                 "rayTraceAndGetMinimum")


def forward_calls(P):
    """(pose, function index, sparse, zdelta) of every fwd_* call, in the order they are recorded."""
    return [(p, fn, sparse, zd) for p in range(P) for fn in range(5) for sparse in (True, False) for zd in (10, 7, 1)]


def run_reverse(B, fx, v=None):
    """The rev_* records: pose, {fast, full}, viz {1, 0}, zdelta {1, 3}; flags reset before each."""
    g = lambda k: fx["in_" + k]
    v = v or make_volume(B, fx)
    eng = B.engine(g("K"), int(g("H")), int(g("W")))
    rev = _Calls(B)
    for T in g("poses").reshape(-1, 12):
        for full in ((0, 1) if int(g("flags")) & 2 else (0,)):
            for viz in (True, False):
                for zd in (1, 3):
                    v.reset_flags()
                    f, lst = (eng.reverseRayTrace if full else eng.reverseRayTraceFast)(v, T, viz, zd)
                    rev.add(v, f, 0, lst)
    return rev.out("rev")


def run_forward(B, fx, v=None):
    """The fwd_*, rtv_* and chain_* records (scenes with bit 1 of flags): pose, function,
    sparse {1, 0}, zdelta {10, 7, 1}."""
    g = lambda k: fx["in_" + k]
    if not int(g("flags")) & 2:
        return {}
    v = v or make_volume(B, fx)
    eng = B.engine(g("K"), int(g("H")), int(g("W")))
    poses = g("poses").reshape(-1, 12)
    fwd, rtv, chain = _Calls(B), _Calls(B), _Calls(B)
    for p, T in enumerate(poses):
        for fn in range(5):
            for sparse in (True, False):
                for zd in (10, 7, 1):
                    v.reset_flags()
                    if fn == 0:
                        eng.rayTrace(v, T, zd, sparse)
                        fwd.add(v)
                    elif fn == 1:
                        eng.rayTraceAndClassify(v, T, zd, p + 1, sparse)
                        fwd.add(v)
                    elif fn == 2:
                        f, lst = eng.rayTraceAndGetGoodPoints(v, T, zd, sparse)
                        fwd.add(v, f, 0, lst)
                    elif fn == 3:
                        f, lst = eng.rayTraceAndGetPoints(v, T, zd, sparse)
                        fwd.add(v, f, 0, lst)
                    else:
                        fwd.add(v, False, eng.rayTraceAndGetMinimum(v, T, zd, sparse))
    for T in poses:
        v.reset_flags()
        eng.rayTraceVolume(v, T)
        rtv.add(v)
    if len(poses) >= 2:
        v.reset_flags()
        eng.rayTraceAndClassify(v, poses[0], 10, 2, False)
        chain.add(v)
        eng.rayTraceAndClassify(v, poses[1], 7, 3, False)
        chain.add(v)
        f, lst = eng.reverseRayTraceFast(v, poses[1], True, 1)
        chain.add(v, f, 0, lst)
    v.reset_flags()
    return {**fwd.out("fwd"), **rtv.out("rtv"), **chain.out("chain")}


def run_core(B, fx):
    """Every record of ref_pin_core, in the driver's order."""
    v = make_volume(B, fx)
    return {**run_volume(B, fx), **run_probes(B, fx), **run_reverse(B, fx, v), **run_forward(B, fx, v)}


def run_ogrid(B, fx):
    g = lambda k: fx["og_in_" + k]
    G = B.ogrid()
    G.setDimensions(*map(float, g("bounds")))
    G.setResolution(*map(float, g("res")))
    G.setK(int(g("k")))
    G.construct()
    cloud, nrm, nf = g("cloud").reshape(-1, 3), g("nrm").reshape(-1, 6), int(g("n_first"))
    G.updateStates(cloud[:nf], nrm[:nf])
    G.updateStates(cloud[nf:], nrm[nf:])
    n, c, cnt, fl = G.state()
    out = {"og_dims": np.array(G.dims, np.int32), "og_normal": n.reshape(-1), "og_centroid": c.reshape(-1),
           "og_count": cnt, "og_flags": fl}
    for name, a in zip(("og_cloud", "og_hq", "og_reorg", "og_reorg_clean"), B.ogrid_downloads(G)):
        out[name] = np.asarray(a, np.float32).reshape(-1)
    return out


def differences(got, exp):
    """Names of the records that differ (bit patterns compared, so NaN == NaN and -0 != 0)."""
    bad = [k for k in exp if k not in got]
    for k, e in exp.items():
        if k in got:
            a = np.ascontiguousarray(got[k])
            if a.dtype != e.dtype or a.shape != e.shape or a.tobytes() != np.ascontiguousarray(e).tobytes():
                bad.append(k)
    return bad + [k for k in got if k not in exp]


def count_differing(got, exp):
    """(entries that differ, entries compared) over all records of equal length, plus records whose
    lengths differ counted whole."""
    nd = nt = 0
    for k, e in exp.items():
        a = got.get(k)
        nt += e.size
        if a is None or a.shape != e.shape:
            nd += e.size
        else:
            nd += int((a.view(np.uint8).reshape(e.size, -1) != e.view(np.uint8).reshape(e.size, -1)).any(1).sum()) if e.size else 0
    return nd, nt
