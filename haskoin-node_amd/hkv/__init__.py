"""hkv — MI355X batch secp256k1 ECDSA verification (host side, ctypes over
the C ABI in ``include/hkv.h``).

This is the Python face of the product path; it loads the in-tree
``haskoin-node_amd/lib/libhkv.so`` (built by ``__graft_entry__.build()``)
and fails loudly when it is missing. There is no CPU fallback.
"""
from .lib import (HKV_BLK_BAD_TX, HKV_BLK_EMPTY, HKV_BLK_MERKLE_OK, HKV_BLK_MUTATED, HKV_HASKOIN, HKV_LIBSECP,
                  HKV_NO_FORKID, HKV_RECORD_SIZE, HKV_SIGHASH_FORKID, HKV_SIGHASH_LEGACY, HKV_TXID_BAD_TX,
                  HKV_TXID_OK, HkvError, HkvTxs, lib_path, load_library)
from .records import make_record, pack_records, unpack_bits
from .headers import check_headers, check_headers_device
from .merkle import merkle_roots, merkle_roots_device
from .blocks import check_blocks, check_blocks_device, split_block, tx_ids, tx_ids_device
from .sighash import TxBatch, tx_sig_hash_batch, verify_std_inputs
from .stdtx import (pack_prevouts, std_tx_jobs_device, tx_verdicts_device, verify_std_txs, verify_std_txs_detail,
                    verify_std_txs_device)
from .blocktx import (HKV_SRC_LIST, HKV_SRC_NONE, block_layout, block_tx_jobs_device, debug_txid_hash_mask,
                      txid_index_device, txid_lookup_device, txid_table_slots, verify_block_txs,
                      verify_block_txs_detail, verify_block_txs_device, verify_block_txs_host)
from .spends import (HKV_SPEND_BALANCED, HKV_SPEND_COINBASE, HKV_SPEND_FIRST, HKV_SPEND_IN_RANGE, HKV_SPEND_OK,
                     HKV_SPEND_OUT_RANGE, HKV_SPEND_RESOLVED, block_spends_device, check_block_txs,
                     debug_spend_stages, spend_table_slots, verify_block_txs_spends_host)
from .chain import (HKV_CHAIN_MIN_DIFFICULTY, HKV_CHAIN_NO_RETARGET, HKV_CHN_ALL, HKV_CHN_BITS_OK,
                    HKV_CHN_CHECKPOINT_OK, HKV_CHN_NOT_FUTURE, HKV_CHN_TIME_OK, HKV_CHN_VERSION_OK, ChainParams,
                    ChainTip, ConnectResult, chain_context_device, chain_ctx, chain_scratch_words, connect_headers,
                    connect_headers_device, debug_chain_stages)
from .chain import PARAMS as CHAIN_PARAMS
from .verify import (Verifier, VerifierConfig, verify_hash_sig_batch,
                     verify_raw_batch)
from .actor import VerifyActor, VerifyActorConfig

__all__ = [
    "HKV_HASKOIN", "HKV_LIBSECP", "HKV_RECORD_SIZE", "HkvError", "lib_path",
    "load_library", "make_record", "pack_records", "unpack_bits", "Verifier",
    "VerifierConfig", "verify_hash_sig_batch", "verify_raw_batch", "HKV_NO_FORKID",
    "HKV_SIGHASH_FORKID", "HKV_SIGHASH_LEGACY", "HkvTxs", "TxBatch", "tx_sig_hash_batch",
    "verify_std_inputs", "check_headers", "check_headers_device",
    "merkle_roots", "merkle_roots_device", "VerifyActor", "VerifyActorConfig",
    "tx_ids", "tx_ids_device", "split_block", "check_blocks", "check_blocks_device",
    "verify_std_txs", "verify_std_txs_detail", "verify_std_txs_device", "std_tx_jobs_device", "tx_verdicts_device",
    "pack_prevouts",
    "verify_block_txs", "verify_block_txs_host", "verify_block_txs_detail", "verify_block_txs_device",
    "block_tx_jobs_device", "txid_index_device", "txid_lookup_device", "txid_table_slots", "block_layout",
    "debug_txid_hash_mask", "HKV_SRC_LIST", "HKV_SRC_NONE",
    "spend_table_slots", "block_spends_device", "verify_block_txs_spends_host", "check_block_txs",
    "debug_spend_stages", "HKV_SPEND_RESOLVED", "HKV_SPEND_FIRST", "HKV_SPEND_IN_RANGE", "HKV_SPEND_OUT_RANGE",
    "HKV_SPEND_BALANCED", "HKV_SPEND_COINBASE", "HKV_SPEND_OK",
    "connect_headers", "connect_headers_device", "chain_context_device", "chain_scratch_words", "chain_ctx",
    "debug_chain_stages", "ChainParams", "ChainTip", "ConnectResult", "CHAIN_PARAMS", "HKV_CHN_TIME_OK",
    "HKV_CHN_NOT_FUTURE", "HKV_CHN_BITS_OK", "HKV_CHN_VERSION_OK", "HKV_CHN_CHECKPOINT_OK", "HKV_CHN_ALL",
    "HKV_CHAIN_NO_RETARGET", "HKV_CHAIN_MIN_DIFFICULTY",
    "HKV_TXID_OK", "HKV_TXID_BAD_TX", "HKV_BLK_MERKLE_OK", "HKV_BLK_MUTATED", "HKV_BLK_BAD_TX", "HKV_BLK_EMPTY",
]
