"""The PGX two-player board games of the reference's registry (envpool/pgx/registration.py), with the same
`register` kwargs (pinned by tests/golden/pgx_registry.json).  Go, the card games, Play2048, Backgammon, the
shogi and chess games and SparrowMahjong are not registered."""
from envpool_amd.registration import register

_BOARD_GAMES = (
    ("TicTacToe-v1", "TicTacToe", "tic_tac_toe"),
    ("ConnectFour-v1", "ConnectFour", "connect_four"),
    ("Hex-v1", "Hex", "hex"),
    ("Othello-v1", "Othello", "othello"),
)

for _task_id, _prefix, _task in _BOARD_GAMES:
    register(task_id=_task_id, import_path="envpool_amd.pgx", spec_cls=f"{_prefix}EnvSpec",
             dm_cls=f"{_prefix}DMEnvPool", gymnasium_cls=f"{_prefix}GymnasiumEnvPool", task=_task,
             max_num_players=2)
