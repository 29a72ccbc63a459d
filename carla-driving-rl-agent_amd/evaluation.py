"""Host side of CARLAgent.evaluate (reference core/carla_agent.py:205-321): the per-step driving metrics of an environment, the
per-trial seed rule and the record written to `evaluation/<agent>/<name>.json`.  numpy only: importable without a GPU."""
import math
import random

import numpy as np

# the six per-trial result lists of the reference's evaluate(), in the order its record is written
RESULT_KEYS = ('collision_rate', 'similarity', 'waypoint_distance', 'speed', 'total_reward', 'timesteps')


def evaluation_info(env):
    """-> (similarity, speed in km/h, distance to the next waypoint, collided) after an environment step.
    An environment with an `evaluation_info()` method answers itself (FakeCARLAEnvironment); otherwise the attributes the reference
    reads are read (core/carla_agent.py:273-275,288): `env.similarity`, the norm of `env.vehicle.get_velocity()` in km/h,
    `env.route.distance_to_next_waypoint()` and `env.should_terminate`."""
    own = getattr(env, 'evaluation_info', None)
    if callable(own):
        similarity, speed, distance, collided = own()
        return float(similarity), float(speed), float(distance), bool(collided)
    v = env.vehicle.get_velocity()
    speed = 3.6 * math.sqrt(v.x ** 2 + v.y ** 2 + v.z ** 2)
    return float(env.similarity), float(speed), float(env.route.distance_to_next_waypoint()), bool(env.should_terminate)


def trial_seed(seeds, trials: int, index: int):
    """The seed of trial `index` (core/carla_agent.py:232-240): a list as long as the number of trials is taken in order, any other
    list is drawn from with `random.choice`, 'sample' draws `random.randint(0, 2**32 - 1)`, None (or anything else) seeds nothing."""
    if isinstance(seeds, list):
        if len(seeds) == trials:
            return seeds[index]
        return random.choice(seeds)
    if isinstance(seeds, str) and seeds == 'sample':
        return random.randint(0, 2 ** 32 - 1)
    return None


def summarize(results: dict) -> dict:
    """Per key of `results` the list itself, `<key>_mean` and `<key>_std` (np.mean / np.std, population), in that order: the record
    the reference writes (core/carla_agent.py:303-312)."""
    record = {}
    for k, v in results.items():
        record[k] = list(v)
        record[f'{k}_mean'] = float(np.mean(v))
        record[f'{k}_std'] = float(np.std(v))
    return record
