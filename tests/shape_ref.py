"""Plain-loop restatement of DESIGN.md section 11 (per-droplet shape and intensity integers), written from the definition
alone: one pixel at a time, Python integers, nothing shared with utils/droplet_shape.py."""

CLASS_OF_CODE = {5: "P1", 7: "P1", 15: "P1", 17: "P1", 25: "P1", 27: "P1", 21: "P2", 33: "P2", 13: "P3", 23: "P3"}


def label_props_ref(labels, gray=None):
    """-> {k: {quantity: int}} for every label k >= 1 that occurs."""
    h, w = len(labels), len(labels[0])

    def lab(y, x):
        return int(labels[y][x]) if 0 <= y < h and 0 <= x < w else None      # None: outside, equal to no label

    def is_border(y, x, k):
        """(y, x) carries label k and one of its 4-neighbours does not."""
        if lab(y, x) != k:
            return False
        return any(lab(y + dy, x + dx) != k for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)))

    out = {}
    for y in range(h):
        for x in range(w):
            k = lab(y, x)
            if k == 0:
                continue
            assert k > 0
            d = out.get(k)
            if d is None:
                d = out[k] = {"area": 0, "Sy": 0, "Sx": 0, "Syy": 0, "Sxx": 0, "Sxy": 0, "min_y": y, "min_x": x, "max_y": y,
                              "max_x": x, "P1": 0, "P2": 0, "P3": 0}
                if gray is not None:
                    d.update(Sg=0, Sgg=0, min_g=int(gray[y][x]), max_g=int(gray[y][x]))
            d["area"] += 1
            d["Sy"] += y
            d["Sx"] += x
            d["Syy"] += y * y
            d["Sxx"] += x * x
            d["Sxy"] += x * y
            d["min_y"], d["max_y"] = min(d["min_y"], y), max(d["max_y"], y)
            d["min_x"], d["max_x"] = min(d["min_x"], x), max(d["max_x"], x)
            if gray is not None:
                g = int(gray[y][x])
                d["Sg"] += g
                d["Sgg"] += g * g
                d["min_g"], d["max_g"] = min(d["min_g"], g), max(d["max_g"], g)
            if is_border(y, x, k):
                code = 1
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if (dy or dx) and is_border(y + dy, x + dx, k):
                            code += 10 if dy and dx else 2
                cls = CLASS_OF_CODE.get(code)
                if cls:
                    d[cls] += 1
    return out
