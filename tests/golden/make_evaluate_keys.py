#!/usr/bin/env python3
"""Generates tests/golden/ref_evaluate_keys.json: the names the reference's CARLAgent.evaluate uses for its results and its logs.

Run in the build container only (`python tests/golden/make_evaluate_keys.py`): it reads the reference's core/carla_agent.py, which
does not exist on the GPU box and is never copied.  The file cannot be imported (TensorFlow, gym, CARLA at module level), so it is
parsed: inside CARLAgent.evaluate the AST is walked for

    results = dict(<key>=[], ...)         -> "results": the keyword names of that literal, in source order
    self.log(<key>=..., ...)              -> "log": the literal keyword names, sorted (a `**{...}` argument has none)

The output holds names only (no program text of the reference)."""
import ast
import json
import os

REF = '/root/reference'
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ref_evaluate_keys.json')


def evaluate_function():
    path = os.path.join(REF, 'core', 'carla_agent.py')
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    for cls in tree.body:
        if isinstance(cls, ast.ClassDef) and cls.name == 'CARLAgent':
            for fn in cls.body:
                if isinstance(fn, ast.FunctionDef) and fn.name == 'evaluate':
                    return fn
    raise AssertionError('CARLAgent.evaluate not found')


def main():
    fn = evaluate_function()
    results, log = None, set()
    for node in ast.walk(fn):
        if (isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name)
                and node.targets[0].id == 'results' and isinstance(node.value, ast.Call)
                and isinstance(node.value.func, ast.Name) and node.value.func.id == 'dict'):
            assert results is None, 'two `results = dict(...)` literals'
            results = [kw.arg for kw in node.value.keywords]
            assert all(results), 'results = dict(**...) has no literal keys'
        if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == 'log'
                and isinstance(node.func.value, ast.Name) and node.func.value.id == 'self'):
            log.update(kw.arg for kw in node.keywords if kw.arg is not None)
    assert results, 'no `results = dict(...)` literal found'
    with open(OUT, 'w') as f:
        json.dump(dict(results=results, log=sorted(log)), f, indent=0)
        f.write('\n')
    print(f'{len(results)} result keys, {len(log)} log keys -> {OUT}')


if __name__ == '__main__':
    main()
