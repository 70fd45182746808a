"""THE DEFINITION of the timecube.Cube stand-in (HAVC_TimeCube's 3D LUT), in numpy: csrc/lut3d.hip equals `lut3d` byte for byte.

UNPINNED: the plugin is not in the reference tree and cannot be executed where the fixtures are made.  Assumptions, all of them this file's: trilinear
interpolation (the plugin's default); the input sample s of an RGB24 clip enters as s / 255; cell and fraction per channel are vsdeoldify_amd.timecube
axis_tables (float32, one operation per step); the eight lattice points around the cell are combined in float32, never fused, by seven
lerp(a, b, f) = a + (b - a) * f per output channel -- four along red with frac_r, two along green with frac_g, one along blue with frac_b; the result is
min(max(v, 0), 1) * 255, rounded half to even.

With an identity table of any size the input comes back byte for byte (test_timecube_host.py runs that on SWEEP_INPUTS inputs)."""
import numpy as np

from vsdeoldify_amd import timecube as TC

f32 = np.float32


def lerp(a, b, f):
    return (a + (b - a) * f).astype(f32)


def lut3d(clip, cube):
    """clip uint8 [..., 3], cube a timecube.Cube -> uint8 of the clip's shape"""
    clip = np.asarray(clip, np.uint8)
    idx, frac = TC.axis_tables(cube)
    table = np.asarray(cube.table, f32)                                                           # [blue][green][red][channel]
    r, g, b = clip[..., 0], clip[..., 1], clip[..., 2]
    ir, ig, ib = idx[0][r], idx[1][g], idx[2][b]
    fr, fg, fb = frac[0][r][..., None], frac[1][g][..., None], frac[2][b][..., None]
    c = lambda db, dg, dr: table[ib + db, ig + dg, ir + dr]                                       # [..., 3]
    r0, r1, r2, r3 = lerp(c(0, 0, 0), c(0, 0, 1), fr), lerp(c(0, 1, 0), c(0, 1, 1), fr), lerp(c(1, 0, 0), c(1, 0, 1), fr), lerp(c(1, 1, 0), c(1, 1, 1), fr)
    v = lerp(lerp(r0, r1, fg), lerp(r2, r3, fg), fb)
    v = (np.minimum(np.maximum(v, f32(0)), f32(1)) * f32(255)).astype(f32)
    return np.rint(v).astype(np.uint8)


def identity_cube(size, domain_min=(0.0, 0.0, 0.0), domain_max=(1.0, 1.0, 1.0)):
    """lattice point i of a channel holds dmin + (dmax - dmin) * i / (N - 1) in float32: the LUT that changes nothing"""
    axes = [(f32(lo) + (f32(hi) - f32(lo)) * (np.arange(size, dtype=f32) / f32(size - 1))).astype(f32) for lo, hi in zip(domain_min, domain_max)]
    table = np.empty((size, size, size, 3), f32)
    table[..., 0] = axes[0][None, None, :]
    table[..., 1] = axes[1][None, :, None]
    table[..., 2] = axes[2][:, None, None]
    return TC.Cube(size, tuple(domain_min), tuple(domain_max), table, "identity")


def random_cube(size, seed=0, lo=-0.2, hi=1.2, domain_min=(0.0, 0.0, 0.0), domain_max=(1.0, 1.0, 1.0)):
    """values in [lo, hi]: the output clamp is hit on both sides"""
    r = np.random.default_rng(1000 * size + seed)
    return TC.Cube(size, tuple(domain_min), tuple(domain_max), r.uniform(lo, hi, (size, size, size, 3)).astype(f32), f"random {seed}")


def graded_cube(size, seed=0):
    """a smooth grade around the identity (a gain, a lift and a channel mix), as a generated stand-in for a shipped look"""
    r = np.random.default_rng(77 + seed)
    ident = identity_cube(size).table.astype(np.float64)
    mix = np.eye(3) + r.uniform(-0.15, 0.15, (3, 3))
    return TC.Cube(size, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (np.power(np.clip(ident @ mix.T, 0, None), 0.9) + r.uniform(-0.03, 0.03, 3)).astype(f32), f"grade {seed}")


def cube_text(cube, line_end="\n", comments=True):
    """the cube as the text of a .cube file"""
    lines = []
    if comments:
        lines += ["# generated for the tests", ""]
    if cube.title:
        lines.append(f'TITLE "{cube.title}"')
    lines.append(f"LUT_3D_SIZE {cube.size}")
    if tuple(cube.domain_min) != (0.0, 0.0, 0.0) or tuple(cube.domain_max) != (1.0, 1.0, 1.0):
        lines.append("DOMAIN_MIN " + " ".join(repr(float(v)) for v in cube.domain_min))
        lines.append("DOMAIN_MAX " + " ".join(repr(float(v)) for v in cube.domain_max))
    if comments:
        lines.append("")
    lines += [" ".join(repr(float(v)) for v in row) for row in np.asarray(cube.table, f32).reshape(-1, 3)]
    return line_end.join(lines) + line_end


def write_cube(path, cube, **kw):
    with open(path, "w", newline="") as f:
        f.write(cube_text(cube, **kw))
    return str(path)


# every (R, G) pair x 36 B values = 2 359 296 inputs, as one frame of 256 x 9216
SWEEP_B = np.unique(np.concatenate([np.arange(0, 256, 8), [1, 127, 129, 255]])).astype(np.uint8)
SWEEP_INPUTS = 256 * 256 * len(SWEEP_B)


def sweep_frame(rotation=0):
    """[256][256 * 36][3]: channel (0 + rotation) % 3 takes every value along the rows, (1 + rotation) % 3 along the columns with (2 + rotation) % 3 through
    SWEEP_B"""
    assert len(SWEEP_B) == 36
    a, b, c = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), SWEEP_B, indexing="ij")
    frame = np.empty((256, 256 * 36, 3), np.uint8)
    for k, plane in enumerate((a, b, c)):
        frame[..., (k + rotation) % 3] = plane.reshape(256, -1)
    return frame


def make_clip(h, w, n, seed=0):
    """seeded noise, every frame different, the last one a smooth gradient"""
    r = np.random.default_rng(31 * h + 7 * w + n + seed)
    clip = r.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    clip[-1] = np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 255) // max(w + h - 2, 1)], -1).astype(np.uint8)
    return clip
