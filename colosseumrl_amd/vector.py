"""Vector-environment adapters over the batched steppers.

The reference exposes single games to RL libraries through ``RllibWrapper`` / ``TronRayEnvironment``
(colosseumrl/envs/wrappers/rllib.py:29-55, envs/tron/rllib.py:30-57): ``reset() -> obs`` and
``step(action_dict) -> obs, rewards, dones, infos`` per agent.  The adapters below give the same
reset/step contract for B games at once, with tensors instead of dicts of Python objects: actions in,
observations / rewards / dones out, everything staying on the GPU, games auto-resetting when they end.
"""
import math
from typing import Dict, Optional, Tuple

import torch

from .batched import BlokusBatch, TronBatch, TTTBatch, _exploration, _int_in, _one_of, _unit, _want


class TronVectorEnv:
    """B simultaneous-move Tron games.  ``step`` takes int8 actions [P, B] in {0 forward, 1 right, -1 left}."""

    def __init__(self, board_size: int = 19, num_players: int = 4, batch: int = 1024, device="cuda"):
        self.batch = TronBatch(board_size, num_players, batch, device=device)
        self.num_players, self.num_envs = num_players, batch

    def observe(self, player: int) -> Dict[str, torch.Tensor]:
        pl = torch.full((self.num_envs,), player, dtype=torch.int8, device=self.batch.device)
        return self.batch.observe(pl)

    def reset(self) -> Dict[int, Dict[str, torch.Tensor]]:
        self.batch.reset()
        return {p: self.observe(p) for p in range(self.num_players)}

    def step(self, actions: torch.Tensor) -> Tuple[Dict[int, Dict[str, torch.Tensor]], torch.Tensor, torch.Tensor, Dict]:
        """-> (obs per player of the state AFTER auto-reset, rewards int8 [P, B], done uint8 [B], info).
        One launch: next_state and the observations of all players come out of the fused ``step_observe`` call."""
        o = self.batch.step_observe(actions, auto_reset=True)
        obs = {p: {"board": o["board"][p], "heads": o["heads"][p], "directions": o["directions"][p], "deaths": o["deaths"][p]}
               for p in range(self.num_players)}
        return obs, o["rewards"].clone(), o["terminal"].clone(), {"winners": o["winners"].clone()}


class TronSinglePlayerVectorEnv:
    """B games of one learner (player 0) against P - 1 scripted opponents: the batched counterpart of the reference's
    ``TronRaySinglePlayerEnvironment`` (envs/tron/rllib.py:98-157) with its default opponent ``SimpleAvoidAgent(noise)``.

    ``reset() -> obs`` and ``step(action) -> obs, reward, done, info`` with ``action`` int64 [B] in {0 forward, 1 right,
    2 left} (the reference's ``action_to_string`` order).  ``obs`` is player 0's relative observation, which for player 0 is
    the state itself: {'board' int8 [B, N, N], 'heads' int16 [P, B], 'directions' int8 [P, B], 'deaths' int8 [P, B]} --
    views of the live state, valid until the next ``step`` / ``reset`` (clone what you keep).  ``reward`` int8 [B] is the
    learner's reward, ``done`` uint8 [B] is "learner dead or game over"; done games restart in the same step and ``obs`` is
    of the state after that restart.  ``info['terminal']`` uint8 [B]: the game itself ended.  ``reward`` / ``done`` /
    ``info`` are buffers rewritten by every step as well.
    A step is two launches (opponents' actions, then step + done + reset) with no host synchronisation, and can be
    captured into a HIP graph (``torch.cuda.graph``).  The opponents' draws follow ``crl_tron_sample_avoid``'s contract
    at each game's step counter, keyed by ``seed``.
    ``opponent="territory"`` puts the opponents on the territory-greedy agent instead (``crl_tron_sample_territory``: the
    first action with the best Voronoi score, with the same ``noise``): only the opponents' sampling launch changes.
    ``opponent="mcts_territory"`` seats the territory tree search (``crl_tron_sample_mcts_territory``,
    ``TronBatch.sample_mcts_territory``'s moves; boards up to 64x64): with probability ``noise`` a uniform action, else the
    most visited action of ``simulations`` descents with ``exploration``, the other players modelled by ``model`` ("random"
    or "avoid") with ``model_noise`` (None: the env's ``noise``).  Still two launches per step; ``simulations`` is at most
    ``TronBatch.mcts_agent_max_simulations`` of the opponents.  The four keywords are checked and otherwise unused with the
    other opponents."""

    OPPONENTS = ("avoid", "territory", "mcts_territory")

    def __init__(self, board_size: int = 15, num_players: int = 4, batch: int = 1024, noise: float = 0.1, seed: int = 0,
                 spawn_offset: int = 2, device="cuda", opponent: str = "avoid", simulations: int = 48,
                 exploration: float = 1.0, model: str = "avoid", model_noise: Optional[float] = None):
        if num_players < 1:
            raise ValueError("num_players must be at least 1")
        if opponent not in self.OPPONENTS:
            raise ValueError("opponent must be 'avoid', 'territory' or 'mcts_territory', got %r" % (opponent,))
        self.opponent = opponent
        _exploration("exploration", exploration)
        _one_of("model", model, ("random", "avoid"))
        self._search = dict(simulations=_int_in("simulations", simulations, 1, 4095), exploration=exploration, agent=model,
                            model_noise=None if model_noise is None else _unit("model_noise", model_noise))
        self.batch = TronBatch(board_size, num_players, batch, device=device, spawn_offset=spawn_offset)
        self.num_players, self.num_envs = num_players, batch
        self.noise, self.seed = float(noise), int(seed)
        if not 0.0 <= self.noise <= 1.0:
            raise ValueError("noise=%r not in [0, 1]" % (noise,))
        if self._search["model_noise"] is None:
            self._search["model_noise"] = self.noise
        dev = self.batch.device
        self._actions = torch.zeros((num_players, batch), dtype=torch.int8, device=dev)
        self._opponents = list(range(1, num_players))
        if opponent == "mcts_territory" and self._opponents:
            _int_in("simulations", simulations, 1, self.batch.mcts_agent_max_simulations(self._opponents))
        self.reward = torch.zeros((batch,), dtype=torch.int8, device=dev)
        self.done = torch.zeros((batch,), dtype=torch.uint8, device=dev)
        self.terminal = torch.zeros((batch,), dtype=torch.uint8, device=dev)

    def observation(self) -> Dict[str, torch.Tensor]:
        b = self.batch
        return {"board": b.board.view(b.B, b.N, b.N), "heads": b.heads, "directions": b.dirs, "deaths": b.deaths}

    def reset(self) -> Dict[str, torch.Tensor]:
        self.batch.reset()
        return self.observation()

    def step(self, action: torch.Tensor) -> Tuple[Dict[str, torch.Tensor], torch.Tensor, torch.Tensor, Dict]:
        b = self.batch
        _want(action, torch.int64, (b.B,), b.device, "action")
        if self._opponents and self.opponent == "mcts_territory":
            b.sample_mcts_territory(seed=self.seed, noise=self.noise, players=self._opponents, out=self._actions, **self._search)
        elif self._opponents:
            sample = b.sample_territory if self.opponent == "territory" else b.sample_avoid
            sample(self.seed, self.noise, players=self._opponents, out=self._actions)
        b.step_single(self._actions, action, self.reward, self.done, self.terminal)
        return self.observation(), self.reward, self.done, {"terminal": self.terminal}

    def flat_mc_action(self, playouts: int, seed: int = 1, max_steps: int = 0, out: Optional[dict] = None) -> torch.Tensor:
        """Flat Monte Carlo for the learner: ``TronBatch.flat_mc_action`` with this env's own setting -- every player on
        the avoid agent with the env's noise, seat 0, each playout ending with the learner's episode
        (``until="seat_done"``), so a row's mean ``ret_sum`` is the expected episode return from here after that action.
        ``seed`` keys the playouts (their draws never coincide with the env's own).  -> int64 [B] in {0, 1, 2}.  No host
        synchronisation; capturable."""
        return self.batch.flat_mc_action(playouts, seed, "avoid", self.noise, None, "seat_done", max_steps, out)

    def territory_action(self, out: Optional[dict] = None) -> torch.Tensor:
        """The territory-greedy action for the learner: ``TronBatch.territory_action`` for seat 0 -- the first action with
        the best Voronoi score (own area minus the best live opponent's).  -> int64 [B] in {0, 1, 2}.  Deterministic; no
        host synchronisation; capturable."""
        return self.batch.territory_action(None, out)

    def mcts_action(self, simulations: int, playouts: int = 16, seed: int = 1, exploration: float = 1.0, max_steps: int = 0,
                    out: Optional[dict] = None) -> torch.Tensor:
        """A tree search for the learner on the env's own games (``TronBatch.mcts_action``): seat 0, the other players
        modelled by the avoid agent with the env's noise -- whatever the env's opponent --, which also plays the playouts.
        ``seed`` keys the search (its draws never coincide with the env's own).  -> int64 [B] in {0, 1, 2} for ``step``,
        one launch, no host synchronisation, capturable.  ``out``: the ``TronBatch.mcts`` dict to reuse (its 'visits' are a
        policy target)."""
        return self.batch.mcts_action(simulations, playouts, seed, exploration, "avoid", self.noise, None, max_steps, out)

    def mcts_territory_action(self, simulations: int, seed: int = 1, exploration: float = 1.0,
                              out: Optional[dict] = None) -> torch.Tensor:
        """``mcts_action`` with Voronoi territory at the leaves (``TronBatch.mcts_territory_action``; boards up to 64x64):
        seat 0, the other players modelled by the avoid agent with the env's noise -- whatever the env's opponent --, a leaf
        valued by one flood of its position, no playouts.  ``seed`` keys the model's draws.  -> int64 [B] in {0, 1, 2} for
        ``step``, one launch, no host synchronisation, capturable.  ``out``: the ``TronBatch.mcts_territory`` dict to
        reuse."""
        return self.batch.mcts_territory_action(simulations, seed, exploration, "avoid", self.noise, None, 256, out)

    def puct_action(self, evaluate, simulations: int, exploration: float = 1.25, fpu: float = 0.5, seed: int = 1,
                    out: Optional[dict] = None) -> torch.Tensor:
        """A tree search valued by the caller's network for the learner on the env's own games (``TronBatch.puct_action``):
        seat 0, the other players modelled by the avoid agent with the env's noise -- whatever the env's opponent --,
        ``evaluate`` the select dict -> (prior, value).  ``seed`` keys the model's draws.  -> int64 [B] in {0, 1, 2} for
        ``step``, two launches per simulation beside the network, no host synchronisation.  ``out``: the ``TronBatch.puct_root``
        dict to reuse (its 'visits' are a policy target)."""
        return self.batch.puct_action(evaluate, simulations, exploration, fpu, seed, "avoid", self.noise, None, out)


class TicTacToeVectorEnv:
    """B turn-based TicTacToe games.  ``step`` takes int8 cell indices [B] for the player to move (-1 = pass)."""

    def __init__(self, dims=(3, 3), k: int = 3, num_players: int = 2, batch: int = 1024, device="cuda"):
        self.batch = TTTBatch(dims, k, num_players, batch, device=device)
        self.num_players, self.num_envs = num_players, batch

    def reset(self):
        self.batch.reset()
        return self.batch.observe(self.batch.to_move), self.batch.to_move.clone(), self.batch.valid_mask()

    def step(self, action: torch.Tensor):
        """-> (obs for the next mover, next mover int8 [B], empties bitmask int32 [B], reward int8 [B] of the
        player who just moved, done uint8 [B], info).  One launch (``TTTBatch.step_observe``)."""
        o = self.batch.step_observe(action, auto_reset=True)
        return ({"board": o["board"]}, o["mover"].clone(), o["valid"], o["reward"].clone(), o["terminal"].clone(),
                {"winners": o["winners"].clone()})


class BlokusVectorEnv:
    """B turn-based Blokus games (4 players, 20x20).  ``step`` takes int32 dense action ids [B] for the player to move
    (``envs.blokus.actions``: ``((piece*400 + y*20 + x)*8 + orientation)*5 + shift``; -1 = pass, the reference's '').
    Like the reference's ``next_state`` it does not validate actions (``match_server`` does, via ``is_valid_action``):
    pick them from ``valid_list`` / ``select`` / ``sample_valid`` (or test them with ``is_valid``)."""

    def __init__(self, batch: int = 1024, device="cuda"):
        self.batch = BlokusBatch(batch, device=device)
        self.num_players, self.num_envs = 4, batch

    def _mover(self) -> torch.Tensor:
        return self.batch.to_move.to(torch.int8)

    def reset(self):
        """-> (obs for the player to move, mover int8 [B], number of legal actions int32 [B])."""
        self.batch.reset()
        mover = self._mover()
        return self.batch.observe(mover), mover, self.batch.valid()

    def valid_mask(self) -> torch.Tensor:
        """Dense legal-action bitmap int32 [B, 10500] of the player to move (42 KB per game: meant for small B)."""
        return self.batch.valid(want_mask=True)[1]

    def valid_list(self, cap: int = 2048, out=None):
        """(count int32 [B], ids int32 [B, cap]): the ORDERED legal action ids of the player to move, compacted -- what the
        reference's ``valid_actions`` returns (BlokusEnvironment.py:453-500), for every game; ``ids[b, :count[b]]`` ascending
        = reference order, -1 beyond.  1,693 is the longest list seen in reference-played games."""
        return self.batch.valid_list(cap, out=out)

    def select(self, rank: torch.Tensor) -> torch.Tensor:
        """Dense id of the rank[b]-th legal action (reference order) of the player to move, -1 where rank is outside
        [0, count): lets a policy that emits an index into the legal list act without materialising the list."""
        return self.batch.select(rank)[0]

    def is_valid(self, action: torch.Tensor) -> torch.Tensor:
        """uint8 [B]: 1 iff action[b] is a legal action of the player to move (``is_valid_action`` for all games)."""
        return self.batch.is_valid(action)

    def sample_valid(self, seed: int = 0) -> torch.Tensor:
        """A uniformly drawn legal action id per game (-1 where the mover must pass)."""
        return self.batch.sample(seed)

    def step(self, action: torch.Tensor, list_cap: int = 0):
        """-> (obs for the next mover, next mover int8 [B], its number of legal actions int32 [B], reward int8 [B] of the
        player who just moved, done uint8 [B], info); finished games restart (obs / mover / counts are of the new game).
        One launch (``BlokusBatch.step_observe``); with ``list_cap`` > 0 a second one right behind it leaves the next mover's
        ordered legal ids in ``info['ids']`` (int32 [B, list_cap], -1 beyond the count)."""
        o = self.batch.step_observe(action, auto_reset=True, list_cap=list_cap)
        obs = {"board": o["board"], "pieces": o["pieces"], "score": o["score"], "player": o["player"]}
        info = {"winners": o["winners"].clone()}
        if list_cap > 0:
            info["ids"] = o["ids"]
        return obs, o["player"].view(-1), o["n_valid"], o["reward"].clone(), o["terminal"].clone(), info


def _seat_tensor(seat, P: int, B: int, device) -> torch.Tensor:
    """int or int8 [B] tensor of seats in [0, P) -> a device int8 [B] tensor the env owns (checked once, here)."""
    if isinstance(seat, torch.Tensor):
        if seat.dtype != torch.int8 or tuple(seat.shape) != (B,):
            raise ValueError("seat must be an int or an int8 tensor of shape (%d,)" % B)
        out = seat.to(device).clone()
        if bool(((out < 0) | (out >= P)).any()):
            raise ValueError("seat values must lie in [0, %d)" % P)
        return out
    if not 0 <= int(seat) < P:
        raise ValueError("seat=%r not in [0, %d)" % (seat, P))
    return torch.full((B,), int(seat), dtype=torch.int8, device=device)


class TicTacToeSinglePlayerVectorEnv:
    """B TicTacToe games of one learner against the random agent in every other seat: the turn-based counterpart of
    ``TronSinglePlayerVectorEnv``.  ``seat`` (an int, or an int8 [B] tensor: a seat per game, so that one learner trains on
    every position) is the learner's player id.

    ``reset() -> obs`` and ``step(action) -> obs, reward, done, info`` with ``action`` int64 [B] a flat cell index (-1 or
    any value outside [0, cells) passes; an occupied cell passes too, as the reference's next_state has it).  Each step
    plays the learner's move and then the random agent until it is the learner's turn again; a game that ends restarts
    in the same step and the opponents before the learner play their first moves of the new game.  ``obs`` = {'board'
    int8 [B, cells]} relative to the learner (reference state_to_observation), ``reward`` int8 [B] is +1 when the learner
    won, -1 when another player won, 0 for a draw or a running game, ``done`` uint8 [B] the game ended in this step,
    ``info`` = {'valid' int32 [B] empties mask of the new state, 'winners' int8 [B]}.  All of them are buffers that the next
    ``step`` / ``reset`` rewrites (clone what you keep).
    A step is ONE launch (``crl_ttt_step_single``) with no host synchronisation, and can be captured into a HIP graph
    (``torch.cuda.graph``).  The opponents' draws are ``crl_ttt_sample``'s at each game's step counter, keyed by ``seed``;
    the learner's ply advances the counter as well.  ``opponent="tactical"`` seats the win-or-block agent with ``noise``
    instead (``crl_ttt_step_single_tactical``, ``TTTBatch.sample_tactical``'s draws): still one launch per step.
    ``opponent="mcts"`` seats the tree search (``crl_ttt_step_single_mcts``, ``TTTBatch.sample_mcts``'s moves) with
    ``simulations`` x ``playouts`` per move, ``exploration`` and ``noise``: one launch per step as well."""

    def __init__(self, dims=(3, 3), k: int = 3, num_players: int = 2, batch: int = 1024, seat=0, seed: int = 0,
                 device="cuda", opponent: str = "random", noise: float = 0.1, simulations: int = 64, playouts: int = 16,
                 exploration: float = 1.0):
        if opponent not in TTTBatch.OPPONENTS:
            raise ValueError("opponent must be 'random', 'tactical' or 'mcts', got %r" % (opponent,))
        self.opponent, self.noise = opponent, _unit("noise", noise)
        self._search = {}
        if opponent == "mcts":
            s_max = min(4095, 65536 // (8 + 2 * max(1, math.prod(int(d) for d in dims))) - 1)      # S_max of crl_ttt_mcts
            _exploration("exploration", exploration)
            self._search = dict(simulations=_int_in("simulations", simulations, 1, s_max),
                                playouts=_int_in("playouts", playouts, 1, 1024), exploration=exploration)
        self.batch = TTTBatch(dims, k, num_players, batch, device=device)
        self.num_players, self.num_envs, self.seed = num_players, batch, int(seed)
        self.seat = _seat_tensor(seat, num_players, batch, self.batch.device)
        self._out = None

    def _step(self, action):
        self._out = self.batch.step_single(self.seat, action, self.seed, out=self._out, opponent=self.opponent, noise=self.noise,
                                           **self._search)
        o = self._out
        return {"board": o["board"]}, o["reward"], o["done"], {"valid": o["valid"], "winners": o["winners"]}

    def reset(self) -> Dict[str, torch.Tensor]:
        self.batch.reset()
        return self._step(None)[0]

    def step(self, action: torch.Tensor):
        _want(action, torch.int64, (self.num_envs,), self.batch.device, "action")
        return self._step(action)

    def mcts_action(self, simulations: int, playouts: int = 16, seed: int = 1, exploration: float = 1.0,
                    out: Optional[dict] = None) -> torch.Tensor:
        """A tree search for the learner on the env's own games (``TTTBatch.mcts_action``): int64 [B] actions for ``step``,
        one launch, no host synchronisation.  It is the learner's turn in every game after ``reset`` / ``step``, so the
        search is the learner's; the tree values every reply, the opponents' included, by random playouts.  ``out``: the
        ``TTTBatch.mcts`` dict to reuse (its 'visits' are a policy target)."""
        return self.batch.mcts_action(simulations, playouts, seed, exploration, out)

    def puct_action(self, evaluate, simulations: int, exploration: float = 1.25, fpu: float = 0.5,
                    out: Optional[dict] = None) -> torch.Tensor:
        """A tree search valued by the caller's network for the learner on the env's own games (``TTTBatch.puct_action``):
        ``evaluate`` takes the leaves (``TTTBatch.puct_select``'s dict) and returns (prior, value).  int64 [B] actions for
        ``step``; two launches per simulation beside the network, no host synchronisation.  ``out``: the ``TTTBatch.puct_root``
        dict to reuse (its 'visits' are a policy target)."""
        return self.batch.puct_action(evaluate, simulations, exploration, fpu, out)


class BlokusSinglePlayerVectorEnv:
    """B Blokus games of one learner against the random agent in the other three seats: the turn-based counterpart of
    ``TronSinglePlayerVectorEnv``.  ``seat`` (an int, or an int8 [B] tensor: a seat per game) is the learner's colour - 1.

    ``reset() -> obs`` and ``step(action) -> obs, reward, done, info`` with ``action`` int64 [B]: with ``action="id"`` a
    dense action id (``envs.blokus.actions``; < 0 passes), placed as the reference's next_state places any action -- pick
    ids from ``info['ids']`` (``list_cap`` > 0) to stay legal; with ``action="rank"`` the index into the learner's ordered
    legal list (``info['n_valid']`` long; outside it = pass), which needs no list at all.  Each step plays the learner's
    move and then the random agent until it is the learner's turn again; a game that ends restarts in the same step.
    ``obs`` = {'board' int8 [B, 20, 20], 'pieces' uint8 [B, 4, 21], 'score' int32 [B, 4]}: the learner's observation
    (reference state_to_observation).  ``reward`` int8 [B] = the learner's rank in the final scores (0 = last, 3 = best:
    the reference's reward at the end of a game) when the game ended, else 0 -- or a ``CRL_BLOKUS_*_ERROR`` code (< 0) for
    an action the reference's next_state raises on, which leaves that game as it was; ``done`` uint8 [B] the game ended;
    ``info`` = {'n_valid' int32 [B] the learner's number of legal actions, 'winners' uint8 [B] bitmask} and, with
    ``list_cap`` > 0, 'ids' int32 [B, list_cap]: the learner's legal ids in the reference's order (only
    ``ids[b, :n_valid[b]]`` is written).  All of them are buffers that the next ``step`` / ``reset`` rewrites.
    A step is ONE launch (``crl_blokus_step_single``; a second, ``crl_blokus_valid_list``, with ``list_cap`` > 0), has no
    host synchronisation and can be captured into a HIP graph.  The opponents' draws are ``crl_blokus_sample``'s at each
    game's step counter, keyed by ``seed``; the learner's ply advances the counter as well.
    ``opponent="mcts"`` seats the tree search in the other three seats (``crl_blokus_step_single_mcts``,
    ``BlokusBatch.sample_mcts``'s moves): with probability ``noise`` the random agent's action, else the most visited child
    of ``simulations`` descents of ``playouts`` playouts each, nodes up to ``width`` children wide, with ``exploration``.
    The step stays one launch.  The five keywords are checked and otherwise unused with the random opponent."""

    def __init__(self, batch: int = 1024, seat=0, seed: int = 0, list_cap: int = 0, action: str = "id", device="cuda",
                 opponent: str = "random", noise: float = 0.0, simulations: int = 64, playouts: int = 1, width: int = 8,
                 exploration: float = 1.0):
        if action not in ("id", "rank"):
            raise ValueError("action must be 'id' or 'rank', not %r" % (action,))
        if list_cap < 0:
            raise ValueError("list_cap must be >= 0")
        self.opponent = _one_of("opponent", opponent, BlokusBatch.OPPONENTS)
        _exploration("exploration", exploration)
        self._search = dict(noise=_unit("noise", noise), simulations=_int_in("simulations", simulations, 1, 1823),   # S_max of crl_blokus_mcts
                            playouts=_int_in("playouts", playouts, 1, 1024), width=_int_in("width", width, 1, 64),
                            exploration=exploration)
        self.batch = BlokusBatch(batch, device=device)
        self.num_players, self.num_envs, self.seed = 4, batch, int(seed)
        self.list_cap, self.rank = int(list_cap), action == "rank"
        self.seat = _seat_tensor(seat, 4, batch, self.batch.device)
        self._out = None
        self._ids = (torch.full((batch, self.list_cap), -1, dtype=torch.int32, device=self.batch.device)
                     if self.list_cap > 0 else None)

    def _step(self, action):
        self._out = self.batch.step_single(self.seat, action, self.seed, rank=self.rank, out=self._out, opponent=self.opponent,
                                           **self._search)
        o = self._out
        info = {"n_valid": o["n_valid"], "winners": o["winners"]}
        if self._ids is not None:
            info["ids"] = self.batch.valid_list(self.list_cap, player=self.seat, out=self._ids)[1]
        return {"board": o["board"], "pieces": o["pieces"], "score": o["score"]}, o["reward"], o["done"], info

    def reset(self) -> Dict[str, torch.Tensor]:
        self.batch.reset()
        return self._step(None)[0]

    def step(self, action: torch.Tensor):
        _want(action, torch.int64, (self.num_envs,), self.batch.device, "action")
        return self._step(action)

    def mcts_action(self, simulations: int, playouts: int = 1, width: int = 8, seed: int = 1, exploration: float = 1.0,
                    candidates: Optional[torch.Tensor] = None) -> torch.Tensor:
        """A tree search with progressive widening for the learner on the env's own games (``BlokusBatch.mcts_action``):
        int64 [B] dense ids for ``step`` (-1 = pass) of an env made with ``action="id"``.  After ``reset`` / ``step`` it is
        the learner's turn in every game, so the searched mover is the learner; every seat below the root plays the
        search's own moves.  One launch, no host synchronisation, capturable."""
        if self.rank:
            raise ValueError("mcts_action returns dense ids: the env must be made with action='id'")
        return self.batch.mcts_action(simulations, playouts, candidates, width, seed, exploration)
