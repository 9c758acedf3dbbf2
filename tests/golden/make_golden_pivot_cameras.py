#!/usr/bin/env python3
"""Pivot-grid camera fixture generator (tests/golden/pivot_cameras.npz).  Runs on the CPU of a development machine with a checkout of the
reference (cvlab-kaist/3DGAN-Inversion):

    python tests/golden/make_golden_pivot_cameras.py REFERENCE_ROOT

Lifts BaseCoach.look_at and BaseCoach.gen_eyes out of training/coaches/base_coach.py by AST (the module itself imports the whole training
stack), binds them to a stand-in object and records look_at(grid_num=5, num='small') -- the three cam2world matrices of
forward(needs_img_grid='small'), fp32 [3,16] -- and gen_eyes(grid_num=5, num='small') [3,3]."""
import ast
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ref_root = sys.argv[1]
    tree = ast.parse(open(os.path.join(ref_root, 'training', 'coaches', 'base_coach.py')).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'BaseCoach'][0]
    funcs = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in ('look_at', 'gen_eyes')]
    assert sorted(f.name for f in funcs) == ['gen_eyes', 'look_at']
    mod = ast.Module(body=funcs, type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = dict(torch=torch, math=math)
    exec(compile(mod, '<lifted base_coach.py>', 'exec'), ns)
    coach = types.SimpleNamespace()
    coach.gen_eyes = types.MethodType(ns['gen_eyes'], coach)
    coach.look_at = types.MethodType(ns['look_at'], coach)
    cams = coach.look_at(grid_num=5, num='small').numpy().astype(np.float32)
    eyes = coach.gen_eyes(grid_num=5, num='small').numpy().astype(np.float32)
    assert cams.shape == (3, 16) and eyes.shape == (3, 3)
    path = os.path.join(HERE, 'pivot_cameras.npz')
    np.savez(path, cams=cams, eyes=eyes)
    print(f'{path}: {os.path.getsize(path)} bytes')
    print(cams)


if __name__ == '__main__':
    main()
