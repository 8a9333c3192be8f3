python -m imitation_amd.scripts.train_rl with seals_ant engine=device hub_install=True
python -m imitation_amd.scripts.train_rl with seals_half_cheetah engine=device hub_install=True
python -m imitation_amd.scripts.train_rl with seals_hopper engine=device hub_install=True
python -m imitation_amd.scripts.train_rl with seals_swimmer engine=device hub_install=True
python -m imitation_amd.scripts.train_rl with seals_walker engine=device hub_install=True
