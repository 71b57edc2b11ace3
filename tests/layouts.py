"""Any of the ten module layouts the fused kernels are compiled for (template parameter F: bit 0 genset, bit 1 battery, bit 2 grid,
bit 3 grid before battery), carved out of ONE generated ``genset+battery+grid`` batch: the columns of the absent modules are
dropped, everything else -- series, parameters, initial state -- is cloned, so the ten batches differ in their module set alone."""
import dataclasses

F_GENSET, F_BATTERY, F_GRID, F_GRID_FIRST = 1, 2, 4, 8
LAYOUTS = (0, 1, 2, 3, 4, 5, 6, 7, 14, 15)
FACTOR_GRID_COLUMNS = ("base_co2", "co2_profile", "tariff", "outage_bits")


def flags_of(layout):
    """The kernels' F of a BatchLayout (one module of every present kind)."""
    return (F_GENSET * layout.has_genset) | (F_BATTERY * layout.has_battery) | (F_GRID * layout.has_grid) \
        | (F_GRID_FIRST * layout.grid_before_battery)


def belongs_to(name):
    """The module kind a column belongs to: "genset" / "battery" / "grid", or None (load, renewable, unbalanced energy)."""
    if name.startswith("gen_"):
        return "genset"
    if name.startswith("bat_") or name in ("charge", "soc"):
        return "battery"
    if name.startswith("grid_") or name in FACTOR_GRID_COLUMNS:
        return "grid"
    return None


def carve(full, flags):
    """A MicrogridBatch of layout ``flags`` with clones of the columns of ``full`` (a ``generate(arch="genset+battery+grid")``
    batch, materialised or factorised) that the layout keeps."""
    from pymgrid_amd import MicrogridBatch
    if flags not in LAYOUTS:
        raise ValueError(f"layout {flags} is not one of {LAYOUTS}")
    L = full.layout
    if not (L.has_genset and L.has_battery and L.has_grid) or L.multi or L.grid_before_battery:
        raise ValueError("carve() starts from a genset+battery+grid batch with one module of every kind")
    has = {"genset": bool(flags & F_GENSET), "battery": bool(flags & F_BATTERY), "grid": bool(flags & F_GRID)}
    layout = dataclasses.replace(L, n_genset=int(has["genset"]), n_battery=int(has["battery"]), n_grid=int(has["grid"]),
                                 grid_before_battery=bool(flags & F_GRID_FIRST))
    cols = {name: t.clone() for name, t in full.cols.items() if has.get(belongs_to(name), True)}
    sub = MicrogridBatch(layout, cols, forecast_noise=full.forecast_noise)
    assert flags_of(sub.layout) == flags, (flags, sub.layout)
    return sub
