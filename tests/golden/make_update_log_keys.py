#!/usr/bin/env python3
"""Generates tests/golden/ref_update_log_keys.json: the names of the scalars the reference logs from inside update().

Run in the build container only (`python tests/golden/make_update_log_keys.py`): it reads the reference's rl/agents/ppo.py and
core/carla_agent.py, which do not exist on the GPU box and are never copied.  Neither file can be imported (TensorFlow, gym, CARLA
at module level), so both are parsed: inside the six functions of the update path --

    PPOAgent.update                       rl/agents/ppo.py
    CARLAgent.update                      core/carla_agent.py
    CARLAgent.apply_policy_gradients      core/carla_agent.py
    CARLAgent.apply_value_gradients       core/carla_agent.py
    CARLAgent.policy_objective            core/carla_agent.py
    CARLAgent.value_objective             core/carla_agent.py

-- every call `self.log(...)` is found by walking the AST and its keyword names are collected.  The output is a sorted list of
names only (no program text of the reference)."""
import ast
import json
import os

REF = '/root/reference'
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ref_update_log_keys.json')
WANTED = {'rl/agents/ppo.py': {'PPOAgent': ('update',)},
          'core/carla_agent.py': {'CARLAgent': ('update', 'apply_policy_gradients', 'apply_value_gradients', 'policy_objective',
                                                'value_objective')}}


def log_keywords(fn: ast.FunctionDef):
    for node in ast.walk(fn):
        if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == 'log'
                and isinstance(node.func.value, ast.Name) and node.func.value.id == 'self'):
            for kw in node.keywords:
                assert kw.arg is not None, f'{fn.name}: self.log(**...) has no literal keys'
                yield kw.arg


def main():
    keys = set()
    for rel, classes in WANTED.items():
        path = os.path.join(REF, rel)
        with open(path) as f:
            tree = ast.parse(f.read(), filename=path)
        for cls in tree.body:
            if isinstance(cls, ast.ClassDef) and cls.name in classes:
                found = {fn.name: fn for fn in cls.body if isinstance(fn, ast.FunctionDef)}
                for name in classes[cls.name]:
                    assert name in found, (rel, cls.name, name)
                    keys.update(log_keywords(found[name]))
    with open(OUT, 'w') as f:
        json.dump(sorted(keys), f, indent=0)
        f.write('\n')
    print(f'{len(keys)} keys -> {OUT}')


if __name__ == '__main__':
    main()
