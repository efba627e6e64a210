"""Compiled models with a NON-CUBIC box, a moved table and other contact parameters: the test models of tests/test_contact_reference_*.py.

Every shipped asset has cube_half = (0.02, 0.02, 0.02): a half size read at the wrong axis -- in the corner signs, the clamp or the
`inside` branch of the narrow phase, or in the slab tests of the renders -- moves no output of the shipped models.  with_contact
replaces the contact-side fields of the desc, as aniso_model.with_inertias replaces the inertias; box / box0 are the canonical models."""
import copy
import dataclasses

import numpy as np

from gym_kmanip_amd.model import MJ_DEFAULT_SOLIMP, MJ_DEFAULT_SOLREF, KModelDesc

BOX_HALF = (0.03, 0.02, 0.012)            # three different half sizes; the shipped cube is (0.02, 0.02, 0.02)


def _unmix(v, default):
    """The geom-side value whose equal-weight mix with MuJoCo's default (model._mix) is v."""
    return [2.0 * float(x) - float(y) for x, y in zip(v, default)]


def with_contact(cm, cube_half=None, table_z=None, table_rect=None, cube_friction=None, frictionloss=None, cube_frictionloss=None,
                 cube_solref=None, cube_solimp=None, def_solref=None, def_solimp=None):
    """A copy of `cm` whose desc has the named fields replaced (None keeps the model's value), and a deep copy of the asset that
    says the same, so tools/mjcf_export.py and the render oracles see the same model.
      cube_half          [3] half sizes of the box (mass and inertia stay: they are independent fields of the desc)
      table_z, table_rect   the table top's height and its rectangle x_lo, x_hi, y_lo, y_hi
      cube_friction      con_cube_friction[0]
      frictionloss       scalar or [nlink]: every joint's friction loss;  cube_frictionloss: the free joint's
      cube_solref / cube_solimp   con_cube_* (the values AFTER MuJoCo's pair mixing: the asset gets the geom-side values that mix to them)
      def_solref / def_solimp     con_def_* (sphere-table pairs, joint limits, friction loss); the asset has no field for MuJoCo's
                                  defaults, so its copy records them under asset["default_contact"]
    With no argument the desc is byte-identical to cm.desc."""
    nl = cm.nlink
    d = KModelDesc.from_buffer_copy(cm.desc)
    asset = copy.deepcopy(cm.asset)
    if cube_half is not None:
        h = [float(x) for x in cube_half]
        assert len(h) == 3 and min(h) > 0
        for k in range(3):
            d.cube_half[k] = h[k]
        asset["cube"]["half_size"] = h
    if table_z is not None:
        d.table_z = float(table_z)
        asset["table"]["plane_z"] = float(table_z)
    if table_rect is not None:
        r = [float(x) for x in table_rect]
        assert len(r) == 4 and r[0] < r[1] and r[2] < r[3]
        for k in range(4):
            d.table_rect[k] = r[k]
        asset["table"]["rect"] = r
    if cube_friction is not None:
        d.con_cube_friction[0] = float(cube_friction)
        asset["cube"]["friction"] = [float(cube_friction)] + list(asset["cube"]["friction"][1:])
    if frictionloss is not None:
        fl = np.broadcast_to(np.asarray(frictionloss, dtype=np.float64), (nl,))
        assert (fl >= 0).all()
        for i in range(nl):
            d.frictionloss[i] = fl[i]
            asset["links"][i]["joint"]["frictionloss"] = float(fl[i])
    if cube_frictionloss is not None:
        assert cube_frictionloss >= 0
        d.cube_frictionloss = float(cube_frictionloss)
        asset["cube"]["frictionloss"] = float(cube_frictionloss)
    for name, val, n, default in (("solref", cube_solref, 2, MJ_DEFAULT_SOLREF), ("solimp", cube_solimp, 5, MJ_DEFAULT_SOLIMP)):
        if val is not None:
            assert len(val) == n
            for k in range(n):
                getattr(d, "con_cube_" + name)[k] = float(val[k])
            asset["cube"][name] = _unmix(val, default)
    for name, val, n in (("solref", def_solref, 2), ("solimp", def_solimp, 5)):
        if val is not None:
            assert len(val) == n
            for k in range(n):
                getattr(d, "con_def_" + name)[k] = float(val[k])
            asset.setdefault("default_contact", {})[name] = [float(x) for x in val]
    return dataclasses.replace(cm, desc=d, asset=asset)


def box(cm):
    """The canonical non-cubic model: cube_half = BOX_HALF, everything else shipped."""
    return with_contact(cm, cube_half=BOX_HALF)


def box0(cm):
    """box with every friction loss zero, joints and cube: qfrc_constraint then holds only contact forces and limit rows (the model
    of the virtual-work check)."""
    return with_contact(cm, cube_half=BOX_HALF, frictionloss=0.0, cube_frictionloss=0.0)
