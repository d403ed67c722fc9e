"""TEST INFRASTRUCTURE ONLY: a numpy restatement of csrc/part_geometry.hip (include/pasta_hip.h, pasta_part_geometry), in scalar
float32 / float64 operations in exactly the kernel's order.  float64 values are Python floats (IEEE doubles, every operation
rounded on its own); float32 values are numpy.float32 scalars.

    quadrilateral   the source quadrilateral of one part [4, 2] float32, or None
    solve           the eight unknowns of perspective_matrix's system by the stated elimination
    inverse         adjugate_inverse's expressions on nine doubles
    geometry        all seven outputs of the kernel for [M, 18, 3] key points
    part_matrices   (fwd, back, valid) in the shape of training.patch_pipeline.part_matrices
    standing_people seeded people as tests/tryon_512_tree.standing_person makes them (halved for 256)"""
import numpy as np

F = np.float32
# joints of training.patch_pipeline.JOINT_ORDER
NOSE, RSHO, RELB, RWRI, LSHO, LELB, LWRI, RHIP, RKNEE, RANK, LHIP, LKNEE, LANK = 0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13
LIMBS = {2: (LSHO, LELB), 3: (LELB, LWRI), 4: (RSHO, RELB), 5: (RELB, RWRI), 6: (LHIP, LKNEE), 7: (LKNEE, LANK), 8: (RHIP, RKNEE), 9: (RKNEE, RANK)}


def _seen(kp, j):
    return float(kp[j, 2]) >= 0.1


def _point(kp, j, x_pad):
    return (F(F(kp[j, 0]) + F(x_pad)), F(kp[j, 1]))


def _box(p, q, ratio):
    sx, sy = F(q[0] - p[0]), F(q[1] - p[1])
    nx, ny = F(F(-sy) * F(ratio)), F(sx * F(ratio))
    return [(F(p[0] + nx), F(p[1] + ny)), (F(p[0] - nx), F(p[1] - ny)), (F(q[0] - nx), F(q[1] - ny)), (F(q[0] + nx), F(q[1] + ny))]


def quadrilateral(kp, part, image_height, x_pad, shin_fallback):
    kp = np.asarray(kp, np.float64)
    with np.errstate(all='ignore'):
        if part == 0:
            if not all(_seen(kp, j) for j in (LSHO, LHIP, RHIP, RSHO)):
                return None
            quad = [_point(kp, j, x_pad) for j in (LSHO, LHIP, RHIP, RSHO)]
        elif part == 1:
            if not (_seen(kp, LSHO) and _seen(kp, RSHO)):
                return None
            p0, p1 = _point(kp, LSHO, x_pad), _point(kp, RSHO, x_pad)
            if not _seen(kp, NOSE):
                sx, sy = F(p1[0] - p0[0]), F(p1[1] - p0[1])
                nx, ny = F(-sy), sx
                if ny > 0:
                    nx, ny = F(-nx), F(-ny)
                quad = [(F(p0[0] + nx), F(p0[1] + ny)), p0, p1, (F(p1[0] + nx), F(p1[1] + ny))]
            else:
                p2 = _point(kp, NOSE, x_pad)
                neck = (F(F(0.5) * F(p0[0] + p1[0])), F(F(0.5) * F(p0[1] + p1[1])))
                top = (F(neck[0] + F(F(2) * F(p2[0] - neck[0]))), F(neck[1] + F(F(2) * F(p2[1] - neck[1]))))
                a, b, c, d = _box(top, neck, 0.5)
                quad = [b, c, d, a]
        else:
            first, second = LIMBS[part]
            if not _seen(kp, first):
                return None
            p = _point(kp, first, x_pad)
            if _seen(kp, second):
                quad = _box(p, _point(kp, second, x_pad), 0.25)
            elif part in (6, 8) or (part in (7, 9) and shin_fallback):
                quad = _box(p, (p[0], F(image_height - 1)), 0.25)
            else:
                return None
    return np.array(quad, np.float32)


def solve(src, dst):
    """[8] floats: perspective_matrix's system for four float32 point pairs, by the elimination of include/pasta_hip.h."""
    a = []
    for (x, y), (u, v) in zip(src, dst):
        x, y, u = float(x), float(y), float(u)
        a.append([x, y, 1.0, 0.0, 0.0, 0.0, -x * u, -y * u, u])
    for (x, y), (u, v) in zip(src, dst):
        x, y, v = float(x), float(y), float(v)
        a.append([0.0, 0.0, 0.0, x, y, 1.0, -x * v, -y * v, v])
    for c in range(8):
        p, best = c, abs(a[c][c])
        for r in range(c + 1, 8):
            if abs(a[r][c]) > best:
                p, best = r, abs(a[r][c])
        if best == 0.0:
            return [0.0] * 8
        a[p], a[c] = a[c], a[p]
        piv = a[c][c]
        for r in range(c + 1, 8):
            m = a[r][c] / piv                   # the pivot is not zero, so Python's division is IEEE's
            row, top = a[r], a[c]
            for k in range(c + 1, 9):
                row[k] = row[k] - m * top[k]
    h = [0.0] * 8
    for r in range(7, -1, -1):
        s = a[r][8]
        for k in range(r + 1, 8):
            s = s - a[r][k] * h[k]
        h[r] = s / a[r][r]
    return h


def inverse(m):
    """adjugate_inverse on nine floats (row-major), in its order."""
    c = [m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
         m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
         m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]]
    det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])
    if det != 0:
        inv = 1.0 / det
        return [v * inv for v in c]
    return [0.0] * 9


def geometry(keypoints, image_height, patch_w, patch_h, x_pad, shin_fallback):
    """dict of the seven outputs of pasta_part_geometry for ``keypoints`` [M, 18, 3]."""
    kp = np.asarray(keypoints, np.float64)
    m = len(kp)
    out = dict(quads=np.zeros([m, 10, 4, 2], np.float32), fwd=np.zeros([m, 10, 9]), back=np.zeros([m, 10, 9]), fwd_inv=np.zeros([m, 10, 9]),
               back_inv=np.zeros([m, 10, 9]), m_inv=np.zeros([m, 10, 9], np.float32), valid=np.zeros([m, 10], np.uint8))
    corners = np.array([[0, 0], [0, patch_h], [patch_w, patch_h], [patch_w, 0]], np.float32)
    for i in range(m):
        for k in range(10):
            quad = quadrilateral(kp[i], k, image_height, x_pad, shin_fallback)
            if quad is None:
                continue
            fwd, back = solve(quad, corners) + [1.0], solve(corners, quad) + [1.0]
            out['quads'][i, k], out['valid'][i, k] = quad, 1
            out['fwd'][i, k], out['back'][i, k] = fwd, back
            out['fwd_inv'][i, k], out['back_inv'][i, k] = inverse(fwd), inverse(back)
            with np.errstate(all='ignore'):
                out['m_inv'][i, k] = np.asarray(back, np.float64).astype(np.float32)
    return out


def part_matrices(joints, width, height, box_factor=2, x_pad=32, shin_fallback=False):
    """training.patch_pipeline.part_matrices with the kernel's rule in place of LAPACK: (fwd, back [N,10,3,3] float64, valid bool)."""
    g = geometry(joints, height, width // 2 ** box_factor, height // 2 ** box_factor, x_pad, shin_fallback)
    n = len(g['valid'])
    return g['fwd'].reshape(n, 10, 3, 3), g['back'].reshape(n, 10, 3, 3), g['valid'].astype(bool)


def standing_people(count, size, seed):
    """[count, 18, 3]: people as tests/tryon_512_tree.standing_person draws them (x, y halved for 256), already on the padded square."""
    from tryon_512_tree import standing_person
    rng = np.random.default_rng(seed)
    people = np.stack([standing_person(rng) for _ in range(count)])
    people[..., 0] += 96.0                      # (512 - 320) / 2
    if size == 256:
        people[..., :2] *= 0.5
    return people


def edge_people(size):
    """[P, 18, 3] people covering every branch of the quadrilateral rule and the solver's edges, on a ``size`` square (x unpadded
    at 256: callers pass x_pad 32 or 0 alike), and what each row is."""
    rng = np.random.default_rng(7)
    from tryon_512_tree import standing_person
    s = size / 512.0

    def person():
        p = standing_person(rng)
        p[:, :2] *= s
        return p
    rows, names = [], []

    def add(name, edit):
        p = person()
        edit(p)
        rows.append(p)
        names.append(name)
    add('complete', lambda p: None)
    add('no left knee', lambda p: p.__setitem__((LKNEE, 2), 0.0))
    add('no right knee, no right hip', lambda p: (p.__setitem__((RKNEE, 2), 0.05), p.__setitem__((RHIP, 2), 0.05)))
    add('no left ankle', lambda p: p.__setitem__((LANK, 2), 0.02))
    add('no right ankle, no right knee', lambda p: (p.__setitem__((RANK, 2), 0.0), p.__setitem__((RKNEE, 2), 0.0)))

    def no_nose(sign):
        def edit(p):
            p[NOSE, 2] = 0.0
            p[LSHO, :2], p[RSHO, :2] = ((204 * s, 124 * s), (116 * s, 130 * s)) if sign > 0 else ((116 * s, 124 * s), (204 * s, 130 * s))
        return edit
    add('no nose, normal[1] < 0', no_nose(-1))
    add('no nose, normal[1] > 0', no_nose(+1))
    add('no left shoulder', lambda p: p.__setitem__((LSHO, 2), 0.0))
    add('no shoulders, no hips', lambda p: p.__setitem__((slice(None), 2), np.where(np.isin(np.arange(18), (RSHO, LSHO, RHIP, LHIP)), 0.05, p[:, 2])))
    add('zero-length right forearm', lambda p: p.__setitem__((RWRI, slice(0, 2)), p[RELB, :2]))
    add('left wrist beyond the canvas', lambda p: p.__setitem__((LWRI, slice(0, 2)), (size * 1.3 + 0.5, 280.25 * s)))
    add('confidence exactly 0.1', lambda p: p.__setitem__((LELB, 2), 0.1))
    add('confidence just below 0.1', lambda p: p.__setitem__((LELB, 2), np.nextafter(0.1, 0.0)))
    add('nobody', lambda p: p.__setitem__((slice(None), 2), 0.0))
    return np.stack(rows), names
