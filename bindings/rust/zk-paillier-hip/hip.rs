//! `zkproofs::hip` — the GPU paths of the hot proofs of zk-paillier, behind cargo feature `hip`.
//!
//! Drop this file in as `src/zkproofs/hip.rs` of ZenGo-X/zk-paillier 0.4.4 and apply `bindings/rust/zk-paillier-hip.patch`
//! (Cargo feature + dependency, `mod hip`, field visibilities, and the five three-line dispatch blocks).  The public API of the
//! crate does not change: `RangeProofNi::{prove, verify, verify_self}`, `NiCorrectKeyProof::verify` and
//! `CompositeDLogProof::{prove, verify}` keep their signatures, results and panics; with the feature on, their inner loops — the
//! 256 / ~192 / 11 / 1-2 modular exponentiations per proof — run in `libzkp_hip.so` (hand-written HIP kernels for MI355X) through
//! the C ABI of `include/zkp_hip.h`, bound by the `zkp-hip-sys` crate.  New here are only the BATCH entry points
//! (`RangeProofNi::prove_batch / verify_batch`, `NiCorrectKeyProof::verify_batch`), which is where a GPU pays off.
//!
//! What goes to the GPU and what stays on GMP
//!   * A proof is CANONICAL when every field is a non-negative integer within its fixed width (n-sized values in n_bits bits,
//!     ciphertexts in 2 n_bits) and it stores exactly `error_factor` rows.  Every honest proof is.  Canonical proofs are flattened
//!     into the structure-of-arrays batch of `zkp_range_ni_proofs` and verified by one `zkp_range_ni_verify_batch`.
//!   * A deserialised proof may hold ANY BigInt (negative, over-wide) and any row count; the reference has a verdict — or a panic —
//!     for each of those.  Such a proof is answered by the crate's own unchanged GMP code (`RangeProof::verifier_output`): the
//!     functions below return `None` and the patched method falls through to the original body.  Same for keys the kernels do not
//!     carry (even, or wider than 4096 bits) and when no gfx950 GPU is present.  So the result is the reference's in every case.
//!   * Verdict byte `ZKP_VERDICT_MALFORMED` = "the reference would panic here" (index out of bounds): the single-proof methods
//!     re-run that proof on the GMP path so that the panic is the reference's own; the batch methods report `Verdict::WouldPanic`.
//!
//! This file is source that has NOT been compiled in the repository it ships from (no rustc there).  `tests/test_rust_bindings.py`
//! checks every `sys::` call below against `include/zkp_hip.h` (name, argument count) and the struct literals against the header.
#![cfg(feature = "hip")]

use std::ptr;
use std::sync::{Mutex, Once};

use curv::arithmetic::traits::*;
use curv::BigInt;
use paillier::EncryptionKey;
use rand::random;
use zkp_hip_sys as sys;

use super::correct_key_ni::NiCorrectKeyProof;
use super::errors::IncorrectProof;
use super::range_proof::{EncryptedPairs, Proof, Response};
use super::range_proof_ni::RangeProofNi;
use super::wi_dlog_proof::{CompositeDLogProof, DLogStatement};

const SECURITY_PARAMETER: usize = sys::ZKP_SECURITY_PARAMETER; // src/zkproofs/range_proof_ni.rs:23
const M2: usize = sys::ZKP_CORRECT_KEY_M2; // src/zkproofs/correct_key_ni.rs:29
const DLOG_Y_BITS: u32 = 768; // an honest y = r + e * s is < 2^513 (wi_dlog_proof.rs:53-62); wider responses take the GMP path

/// Outcome of one proof of a batch call.
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum Verdict {
    /// `Ok(())`
    Accept,
    /// `Err(IncorrectProof)`
    Reject,
    /// the reference panics on this proof (index out of bounds / assert): call the single-proof method to get that panic
    WouldPanic,
}

impl Verdict {
    pub fn into_result(self) -> Result<(), IncorrectProof> {
        match self {
            Verdict::Accept => Ok(()),
            Verdict::Reject => Err(IncorrectProof),
            Verdict::WouldPanic => panic!("malformed proof: the reference implementation panics on it"),
        }
    }
}

// ------------------------------------------------------------------------------------------------ context
struct Ctx(*mut sys::zkp_ctx);
// one ctx = one GPU + one stream; calls on it are serialised by the Mutex below (include/zkp_hip.h, "Conventions")
unsafe impl Send for Ctx {}

static INIT: Once = Once::new();
static mut CTX: Option<Mutex<Ctx>> = None;

/// The process-wide engine context on GPU `ZKP_HIP_DEVICE` (default 0); `None` when there is no gfx950 device — the crate then
/// keeps computing on GMP (libzkp_hip.so itself has no CPU fallback: zkp_ctx_create fails with ZKP_EDEVICE).
fn with_ctx<T>(f: impl FnOnce(*mut sys::zkp_ctx) -> Option<T>) -> Option<T> {
    INIT.call_once(|| {
        let device = std::env::var("ZKP_HIP_DEVICE").ok().and_then(|s| s.parse::<i32>().ok()).unwrap_or(0);
        let mut raw: *mut sys::zkp_ctx = ptr::null_mut();
        let st = unsafe { sys::zkp_ctx_create(device, &mut raw) };
        if st == sys::ZKP_OK && !raw.is_null() {
            unsafe { CTX = Some(Mutex::new(Ctx(raw))) };
        }
    });
    let cell = unsafe { CTX.as_ref() }?;
    let guard = cell.lock().ok()?;
    f(guard.0)
}

fn ok(status: i32) -> Option<()> {
    if status == sys::ZKP_OK {
        Some(())
    } else {
        None // ZKP_ENONCANONICAL (even modulus), ZKP_EDEVICE, ...: the caller falls back to GMP
    }
}

// ------------------------------------------------------------------------------------------------ BigInt <-> limbs
/// kernel width for an n of this size (include/zkp_hip.h: n_bits in {1024, 2048, 4096}); `None` for keys the kernels do not carry
fn width_for(n: &BigInt) -> Option<u32> {
    if BigInt::is_negative(n) || n.is_even() {
        return None;
    }
    match n.bit_length() {
        0..=1 => None,
        2..=1024 => Some(1024),
        1025..=2048 => Some(2048),
        2049..=4096 => Some(4096),
        _ => None,
    }
}

/// fixed-width little-endian 32-bit limbs (the ABI's integer form); false if `x` is negative or does not fit: not canonical
fn put_limbs(dst: &mut [u32], x: &BigInt) -> bool {
    if BigInt::is_negative(x) {
        return false;
    }
    let be = BigInt::to_bytes(x); // minimal big-endian magnitude, zero -> [0]
    if be.len() > 4 * dst.len() {
        return false;
    }
    for w in dst.iter_mut() {
        *w = 0;
    }
    for (i, b) in be.iter().rev().enumerate() {
        dst[i / 4] |= (*b as u32) << (8 * (i % 4));
    }
    true
}

fn get_limbs(src: &[u32]) -> BigInt {
    let mut be = Vec::with_capacity(4 * src.len());
    for w in src.iter().rev() {
        be.extend_from_slice(&w.to_be_bytes());
    }
    BigInt::from_bytes(&be)
}

// ------------------------------------------------------------------------------------------------ RangeProofNi
/// The structure-of-arrays batch of include/zkp_hip.h (`zkp_range_ni_proofs`), owned.
struct RangeBatch {
    n_bits: u32,
    ef: usize,
    b: usize,
    n: Vec<u32>,
    range: Vec<u32>,
    ciphertext: Vec<u32>,
    c1: Vec<u32>,
    c2: Vec<u32>,
    kind: Vec<u8>,
    j: Vec<u8>,
    w1: Vec<u32>,
    r1: Vec<u32>,
    w2: Vec<u32>,
    r2: Vec<u32>,
}

impl RangeBatch {
    fn new(n_bits: u32, b: usize, ef: usize) -> RangeBatch {
        let kw = (n_bits / 32) as usize;
        RangeBatch {
            n_bits,
            ef,
            b,
            n: vec![0; kw],
            range: vec![0; b * kw],
            ciphertext: vec![0; b * 2 * kw],
            c1: vec![0; b * ef * 2 * kw],
            c2: vec![0; b * ef * 2 * kw],
            kind: vec![0; b * ef],
            j: vec![0; b * ef],
            w1: vec![0; b * ef * kw],
            r1: vec![0; b * ef * kw],
            w2: vec![0; b * ef * kw],
            r2: vec![0; b * ef * kw],
        }
    }

    /// one shared key for the whole batch: n_stride = 0
    fn raw(&mut self) -> sys::zkp_range_ni_proofs {
        sys::zkp_range_ni_proofs {
            n_bits: self.n_bits,
            error_factor: self.ef as u32,
            batch: self.b as u64,
            n_stride: 0,
            n: self.n.as_ptr(),
            range: self.range.as_ptr(),
            ciphertext: self.ciphertext.as_ptr(),
            c1: self.c1.as_mut_ptr(),
            c2: self.c2.as_mut_ptr(),
            resp_kind: self.kind.as_mut_ptr(),
            resp_j: self.j.as_mut_ptr(),
            resp_w1: self.w1.as_mut_ptr(),
            resp_r1: self.r1.as_mut_ptr(),
            resp_w2: self.w2.as_mut_ptr(),
            resp_r2: self.r2.as_mut_ptr(),
        }
    }

    /// proof `b` of the batch as the crate's types (after a prove call)
    fn proof(&self, b: usize) -> (EncryptedPairs, Proof) {
        let kw = (self.n_bits / 32) as usize;
        let mut pairs = EncryptedPairs { c1: Vec::with_capacity(self.ef), c2: Vec::with_capacity(self.ef) };
        let mut responses = Vec::with_capacity(self.ef);
        for i in 0..self.ef {
            let t = b * self.ef + i;
            pairs.c1.push(get_limbs(&self.c1[t * 2 * kw..(t + 1) * 2 * kw]));
            pairs.c2.push(get_limbs(&self.c2[t * 2 * kw..(t + 1) * 2 * kw]));
            let lo = t * kw;
            let hi = lo + kw;
            if self.kind[t] == sys::ZKP_RESP_OPEN {
                responses.push(Response::Open {
                    w1: get_limbs(&self.w1[lo..hi]),
                    r1: get_limbs(&self.r1[lo..hi]),
                    w2: get_limbs(&self.w2[lo..hi]),
                    r2: get_limbs(&self.r2[lo..hi]),
                });
            } else {
                responses.push(Response::Mask {
                    j: self.j[t],
                    masked_x: get_limbs(&self.w1[lo..hi]),
                    masked_r: get_limbs(&self.r1[lo..hi]),
                });
            }
        }
        (pairs, Proof(responses))
    }

    /// flattens `p` into slot `b`; false when the proof is not canonical (then nothing of the batch may be used for it)
    fn fill(&mut self, b: usize, p: &RangeProofNi) -> bool {
        let kw = (self.n_bits / 32) as usize;
        let ef = self.ef;
        if p.error_factor != ef || p.proof.0.len() != ef || p.encrypted_pairs.c1.len() != ef || p.encrypted_pairs.c2.len() != ef {
            return false;
        }
        if get_limbs(&self.n) != p.ek.n {
            return false; // RangeProofNi::verify asserts the verifier's key is the proof's (range_proof_ni.rs:86): GMP path, which panics there
        }
        if !put_limbs(&mut self.range[b * kw..(b + 1) * kw], &p.range) || !put_limbs(&mut self.ciphertext[b * 2 * kw..(b + 1) * 2 * kw], &p.ciphertext) {
            return false;
        }
        for i in 0..ef {
            let t = b * ef + i;
            if !put_limbs(&mut self.c1[t * 2 * kw..(t + 1) * 2 * kw], &p.encrypted_pairs.c1[i]) || !put_limbs(&mut self.c2[t * 2 * kw..(t + 1) * 2 * kw], &p.encrypted_pairs.c2[i]) {
                return false;
            }
            let lo = t * kw;
            let hi = lo + kw;
            let fits = match &p.proof.0[i] {
                Response::Open { w1, r1, w2, r2 } => {
                    self.kind[t] = sys::ZKP_RESP_OPEN;
                    self.j[t] = 0;
                    put_limbs(&mut self.w1[lo..hi], w1) && put_limbs(&mut self.r1[lo..hi], r1) && put_limbs(&mut self.w2[lo..hi], w2) && put_limbs(&mut self.r2[lo..hi], r2)
                }
                Response::Mask { j, masked_x, masked_r } => {
                    self.kind[t] = sys::ZKP_RESP_MASK;
                    self.j[t] = *j;
                    put_limbs(&mut self.w1[lo..hi], masked_x) && put_limbs(&mut self.r1[lo..hi], masked_r)
                }
            };
            if !fits {
                return false;
            }
        }
        true
    }
}

/// One prover's statement and witness for `RangeProofNi::prove_batch`.
pub struct RangeStatement<'a> {
    pub range: &'a BigInt,
    pub ciphertext: &'a BigInt,
    pub secret_x: &'a BigInt,
    pub secret_r: &'a BigInt,
}

/// `RangeProofNi::prove` (src/zkproofs/range_proof_ni.rs:47-82) for many provers under one key: the randomness is drawn exactly as
/// `RangeProof::generate_encrypted_pairs` draws it (range_proof.rs:133-159), then ONE `zkp_range_ni_prove_batch` computes the
/// 256 encryptions per proof (range_proof.rs:161-187), the Fiat-Shamir challenge (range_proof_ni.rs:58-61, utils.rs:9-22) and the
/// responses (range_proof.rs:210-252).  `None`: not representable / no GPU — prove on GMP instead.
pub fn range_ni_prove_batch(ek: &EncryptionKey, statements: &[RangeStatement]) -> Option<Vec<RangeProofNi>> {
    let n_bits = width_for(&ek.n)?;
    let kw = (n_bits / 32) as usize;
    let b = statements.len();
    let ef = SECURITY_PARAMETER;
    if b == 0 {
        return Some(Vec::new());
    }
    let mut batch = RangeBatch::new(n_bits, b, ef);
    if !put_limbs(&mut batch.n, &ek.n) {
        return None;
    }
    let (mut x, mut r) = (vec![0u32; b * kw], vec![0u32; b * kw]);
    let (mut w1, mut w2, mut r1, mut r2) = (vec![0u32; b * ef * kw], vec![0u32; b * ef * kw], vec![0u32; b * ef * kw], vec![0u32; b * ef * kw]);
    for (k, st) in statements.iter().enumerate() {
        if !put_limbs(&mut batch.range[k * kw..(k + 1) * kw], st.range)
            || !put_limbs(&mut batch.ciphertext[k * 2 * kw..(k + 1) * 2 * kw], st.ciphertext)
            || !put_limbs(&mut x[k * kw..(k + 1) * kw], st.secret_x)
            || !put_limbs(&mut r[k * kw..(k + 1) * kw], st.secret_r)
        {
            return None;
        }
        let range_scaled_third = st.range.div_floor(&BigInt::from(3)); // range_proof.rs:133
        let range_scaled_two_thirds = BigInt::from(2) * &range_scaled_third; // :134
        for i in 0..ef {
            let t = k * ef + i;
            let mut a = BigInt::sample_range(&range_scaled_third, &range_scaled_two_thirds); // :136-139
            let mut c = &a - &range_scaled_third; // :141
            if random() {
                std::mem::swap(&mut a, &mut c); // :144-149
            }
            if !put_limbs(&mut w1[t * kw..(t + 1) * kw], &a)
                || !put_limbs(&mut w2[t * kw..(t + 1) * kw], &c)
                || !put_limbs(&mut r1[t * kw..(t + 1) * kw], &BigInt::sample_below(&ek.n)) // :151-154
                || !put_limbs(&mut r2[t * kw..(t + 1) * kw], &BigInt::sample_below(&ek.n)) // :156-159
            {
                return None;
            }
        }
    }
    let witness = sys::zkp_range_ni_witness { x: x.as_ptr(), r: r.as_ptr(), w1: w1.as_ptr(), w2: w2.as_ptr(), r1: r1.as_ptr(), r2: r2.as_ptr() };
    let mut status = vec![0u8; b];
    let raw = batch.raw();
    with_ctx(|ctx| ok(unsafe { sys::zkp_range_ni_prove_batch(ctx, &raw, &witness, ptr::null_mut(), ptr::null_mut(), status.as_mut_ptr(), 0) }))?;
    if status.iter().any(|s| *s != 0) {
        return None; // a row the fixed width cannot carry (x + w wider than the key): GMP decides
    }
    let mut out = Vec::with_capacity(b);
    for (k, st) in statements.iter().enumerate() {
        let (encrypted_pairs, proof) = batch.proof(k);
        out.push(RangeProofNi {
            ek: ek.clone(),
            range: st.range.clone(),
            ciphertext: st.ciphertext.clone(),
            encrypted_pairs,
            proof,
            error_factor: SECURITY_PARAMETER,
        });
    }
    Some(out)
}

/// The same from what `RangeProofNi::prove` takes — statements and secrets only: a fresh 32-byte seed from the crate's RNG (`rand::random`,
/// the source `generate_encrypted_pairs` draws its coins from) is expanded into (w1, w2, r1, r2) ON THE GPU by
/// `zkp_range_ni_prove_seeded_batch` (the stream is published in include/zkp_hip.h).  No witness is sampled through GMP, flattened or
/// uploaded, and none is left on the host; the seed — worth the whole witness — is overwritten before this returns and never reused.
pub fn range_ni_prove_seeded_batch(ek: &EncryptionKey, statements: &[RangeStatement]) -> Option<Vec<RangeProofNi>> {
    let n_bits = width_for(&ek.n)?;
    let kw = (n_bits / 32) as usize;
    let b = statements.len();
    let ef = SECURITY_PARAMETER;
    if b == 0 {
        return Some(Vec::new());
    }
    let mut batch = RangeBatch::new(n_bits, b, ef);
    if !put_limbs(&mut batch.n, &ek.n) {
        return None;
    }
    let (mut x, mut r) = (vec![0u32; b * kw], vec![0u32; b * kw]);
    for (k, st) in statements.iter().enumerate() {
        if !put_limbs(&mut batch.range[k * kw..(k + 1) * kw], st.range)
            || !put_limbs(&mut batch.ciphertext[k * 2 * kw..(k + 1) * 2 * kw], st.ciphertext)
            || !put_limbs(&mut x[k * kw..(k + 1) * kw], st.secret_x)
            || !put_limbs(&mut r[k * kw..(k + 1) * kw], st.secret_r)
        {
            return None;
        }
    }
    let mut seed: [u8; 32] = random();
    let mut status = vec![0u8; b];
    let raw = batch.raw();
    let done = with_ctx(|ctx| {
        ok(unsafe { sys::zkp_range_ni_prove_seeded_batch(ctx, &raw, x.as_ptr(), r.as_ptr(), seed.as_ptr(), 0, ptr::null_mut(), ptr::null_mut(), status.as_mut_ptr(), 0) })
    });
    for byte in seed.iter_mut() {
        unsafe { ptr::write_volatile(byte, 0) };
    }
    done?;
    if status.iter().any(|s| *s != 0) {
        return None; // an empty interval (range < 3) or a row the fixed width cannot carry: GMP decides
    }
    let mut out = Vec::with_capacity(b);
    for (k, st) in statements.iter().enumerate() {
        let (encrypted_pairs, proof) = batch.proof(k);
        out.push(RangeProofNi {
            ek: ek.clone(),
            range: st.range.clone(),
            ciphertext: st.ciphertext.clone(),
            encrypted_pairs,
            proof,
            error_factor: SECURITY_PARAMETER,
        });
    }
    Some(out)
}

/// `RangeProofNi::verify_self` (range_proof_ni.rs:109-128 -> range_proof.rs:254-355) for many proofs under one key.
/// Entry k is `None` when proof k has to be decided by the GMP path (not canonical, see the module docs); the whole result is
/// `None` when the key is not one the kernels carry or there is no GPU.
pub fn range_ni_verify_batch(ek: &EncryptionKey, proofs: &[&RangeProofNi]) -> Option<Vec<Option<Verdict>>> {
    let n_bits = width_for(&ek.n)?;
    if proofs.is_empty() {
        return Some(Vec::new());
    }
    let ef = proofs[0].error_factor;
    if ef == 0 || ef > 256 {
        return None;
    }
    // canonical proofs are packed densely; `slot[k]` is the position of proof k in the launch
    let mut slot: Vec<Option<usize>> = Vec::with_capacity(proofs.len());
    let mut batch = RangeBatch::new(n_bits, proofs.len(), ef);
    if !put_limbs(&mut batch.n, &ek.n) {
        return None;
    }
    let mut used = 0usize;
    for p in proofs.iter() {
        if batch.fill(used, p) {
            slot.push(Some(used));
            used += 1;
        } else {
            slot.push(None);
        }
    }
    let mut verdict = vec![9u8; used];
    if used > 0 {
        batch.b = used;
        let raw = batch.raw();
        with_ctx(|ctx| ok(unsafe { sys::zkp_range_ni_verify_batch(ctx, &raw, verdict.as_mut_ptr(), 0) }))?;
    }
    Some(
        slot.iter()
            .map(|s| {
                s.map(|i| match verdict[i] {
                    sys::ZKP_VERDICT_ACCEPT => Verdict::Accept,
                    sys::ZKP_VERDICT_REJECT => Verdict::Reject,
                    _ => Verdict::WouldPanic,
                })
            })
            .collect(),
    )
}

/// `serde_json::to_string(proof)` for many proofs under one key: radix conversion, sizing and assembly of the documents run on the GPU
/// (`zkp_json_write_range_proof_ni_batch`), the text comes back finished.  `key_form` / `bare_form`: `sys::ZKP_BIGINT_DEC` / `_HEX` /
/// `_BYTES`, the text forms of `ek.n` and of `range` / `ciphertext` in this build of curv and kzen-paillier.  `None` when the GPU cannot
/// take the batch (another key, a value the fixed width cannot carry, no device): the caller then writes with serde.
pub fn to_json_batch(ek: &EncryptionKey, proofs: &[&RangeProofNi], key_form: u32, bare_form: u32) -> Option<Vec<String>> {
    let n_bits = width_for(&ek.n)?;
    if proofs.is_empty() {
        return Some(Vec::new());
    }
    let ef = proofs[0].error_factor;
    if ef == 0 || ef > 256 {
        return None;
    }
    let mut batch = RangeBatch::new(n_bits, proofs.len(), ef);
    if !put_limbs(&mut batch.n, &ek.n) {
        return None;
    }
    for (k, p) in proofs.iter().enumerate() {
        if p.ek.n != ek.n || !batch.fill(k, p) {
            return None;
        }
    }
    let raw = batch.raw();
    let forms = (key_form << 4) | bare_form;
    let mut off = vec![0u64; proofs.len() + 1];
    // the sizing call, one allocation, the writing call
    with_ctx(|ctx| ok(unsafe { sys::zkp_json_write_range_proof_ni_batch(ctx, &raw, forms, ptr::null_mut(), 0, off.as_mut_ptr(), ptr::null_mut(), 0) }))?;
    let mut text = vec![0u8; off[proofs.len()] as usize];
    let cap = text.len() as u64;
    with_ctx(|ctx| ok(unsafe { sys::zkp_json_write_range_proof_ni_batch(ctx, &raw, forms, text.as_mut_ptr() as *mut std::os::raw::c_char, cap, off.as_mut_ptr(), ptr::null_mut(), 0) }))?;
    let mut docs = Vec::with_capacity(proofs.len());
    for k in 0..proofs.len() {
        docs.push(String::from_utf8(text[off[k] as usize..off[k + 1] as usize].to_vec()).ok()?);
    }
    Some(docs)
}

impl RangeProofNi {
    /// Many provers, one key, one GPU launch sequence.  Falls back to `RangeProofNi::prove` per statement (whose own dispatch ends
    /// in the original GMP body) when the GPU cannot take the batch.
    pub fn prove_batch(ek: &EncryptionKey, statements: &[RangeStatement]) -> Vec<RangeProofNi> {
        match range_ni_prove_batch(ek, statements) {
            Some(v) => v,
            None => statements.iter().map(|s| RangeProofNi::prove(ek, s.range, s.ciphertext, s.secret_x, s.secret_r)).collect(),
        }
    }

    /// `prove_batch` with the witness expanded on the GPU from a fresh seed (`range_ni_prove_seeded_batch`); the same fall-back.
    pub fn prove_seeded(ek: &EncryptionKey, statements: &[RangeStatement]) -> Vec<RangeProofNi> {
        match range_ni_prove_seeded_batch(ek, statements) {
            Some(v) => v,
            None => statements.iter().map(|s| RangeProofNi::prove(ek, s.range, s.ciphertext, s.secret_x, s.secret_r)).collect(),
        }
    }

    /// `proof.verify(ek, &proof.ciphertext)` for many proofs under the verifier's key `ek`; proofs the GPU path does not take are
    /// verified by the crate's GMP code (a proof under another key panics there, as range_proof_ni.rs:86 does), so every entry is the
    /// reference's outcome.
    pub fn verify_batch(ek: &EncryptionKey, proofs: &[&RangeProofNi]) -> Vec<Verdict> {
        let gpu = range_ni_verify_batch(ek, proofs);
        proofs
            .iter()
            .enumerate()
            .map(|(k, p)| match gpu.as_ref().and_then(|v| v[k]) {
                Some(v) => v,
                None => match std::panic::catch_unwind(std::panic::AssertUnwindSafe(|| p.verify(ek, &p.ciphertext))) {
                    Ok(Ok(())) => Verdict::Accept,
                    Ok(Err(IncorrectProof)) => Verdict::Reject,
                    Err(_) => Verdict::WouldPanic,
                },
            })
            .collect()
    }
}

/// Single-proof dispatch used by the patched `RangeProofNi::{verify, verify_self}`: `Some(result)` when the GPU decided,
/// `None` -> run the original body (non-canonical proof, unsupported key, no GPU, or a proof the reference panics on: the GMP
/// path then produces that very panic).
pub fn range_ni_verify_one(ek: &EncryptionKey, proof: &RangeProofNi) -> Option<Result<(), IncorrectProof>> {
    match range_ni_verify_batch(ek, &[proof])?.pop()?? {
        Verdict::Accept => Some(Ok(())),
        Verdict::Reject => Some(Err(IncorrectProof)),
        Verdict::WouldPanic => None,
    }
}

/// Single-proof dispatch used by the patched `RangeProofNi::prove`.
pub fn range_ni_prove_one(ek: &EncryptionKey, range: &BigInt, ciphertext: &BigInt, secret_x: &BigInt, secret_r: &BigInt) -> Option<RangeProofNi> {
    range_ni_prove_batch(ek, &[RangeStatement { range, ciphertext, secret_x, secret_r }])?.pop()
}

// ------------------------------------------------------------------------------------------------ NiCorrectKeyProof
/// `NiCorrectKeyProof::verify` (src/zkproofs/correct_key_ni.rs:73-100) for many (key, proof) pairs: the SHA-256 mask generation
/// (:77-86, 105-117), the 11 sigma_i^n mod n (:90-93) and gcd(primorial, n) (:87-88) all run in `zkp_correct_key_ni_verify_batch`.
/// Keys must share one width; `None` entries / result as for the range proof.
pub fn correct_key_ni_verify_batch(items: &[(&EncryptionKey, &NiCorrectKeyProof)], salt: &[u8]) -> Option<Vec<Option<Verdict>>> {
    if items.is_empty() {
        return Some(Vec::new());
    }
    let n_bits = width_for(&items[0].0.n)?;
    let kw = (n_bits / 32) as usize;
    let mut slot: Vec<Option<usize>> = Vec::with_capacity(items.len());
    let (mut n, mut sigma) = (Vec::<u32>::new(), Vec::<u32>::new());
    let mut used = 0usize;
    for (ek, proof) in items.iter() {
        // sigma_vec[i] for i < 11: a shorter vector is an index panic in the reference (:92), a longer one is read up to 11
        let mut row_n = vec![0u32; kw];
        let mut row_s = vec![0u32; M2 * kw];
        let fits = width_for(&ek.n) == Some(n_bits)
            && proof.sigma_vec.len() >= M2
            && put_limbs(&mut row_n, &ek.n)
            && (0..M2).all(|i| put_limbs(&mut row_s[i * kw..(i + 1) * kw], &proof.sigma_vec[i]));
        if fits {
            n.extend_from_slice(&row_n);
            sigma.extend_from_slice(&row_s);
            slot.push(Some(used));
            used += 1;
        } else {
            slot.push(None);
        }
    }
    let mut verdict = vec![9u8; used];
    if used > 0 {
        with_ctx(|ctx| {
            ok(unsafe {
                sys::zkp_correct_key_ni_verify_batch(ctx, n_bits, used as u64, n.as_ptr(), sigma.as_ptr(), salt.as_ptr(), salt.len() as u32, verdict.as_mut_ptr(), 0)
            })
        })?;
    }
    Some(
        slot.iter()
            .map(|s| s.map(|i| if verdict[i] == sys::ZKP_VERDICT_ACCEPT { Verdict::Accept } else if verdict[i] == sys::ZKP_VERDICT_REJECT { Verdict::Reject } else { Verdict::WouldPanic }))
            .collect(),
    )
}

/// `serde_json::from_str::<NiCorrectKeyProof>` + `verify` for many (key, document) pairs in ONE `zkp_correct_key_ni_verify_json_batch`: the
/// text is tokenised, converted and verified on the GPU.  Keys must share one width.  `None` for a pair: the key does not fit that width, or
/// the document was not converted (`ZKP_DOC_INVALID`: serde's error; `ZKP_DOC_HOST_PATH`: a root the fixed layout cannot carry) — the caller
/// keeps it on its serde + CPU path.
pub fn correct_key_ni_verify_json_batch(items: &[(&EncryptionKey, &str)], salt: &[u8]) -> Option<Vec<Option<Verdict>>> {
    if items.is_empty() {
        return Some(Vec::new());
    }
    let n_bits = width_for(&items[0].0.n)?;
    let kw = (n_bits / 32) as usize;
    let mut slot: Vec<Option<usize>> = Vec::with_capacity(items.len());
    let (mut n, mut text) = (Vec::<u32>::new(), Vec::<u8>::new());
    let (mut off, mut len) = (Vec::<u64>::new(), Vec::<u64>::new());
    for (ek, doc) in items.iter() {
        let mut row_n = vec![0u32; kw];
        if width_for(&ek.n) == Some(n_bits) && put_limbs(&mut row_n, &ek.n) {
            n.extend_from_slice(&row_n);
            off.push(text.len() as u64);
            len.push(doc.len() as u64);
            text.extend_from_slice(doc.as_bytes());
            slot.push(Some(off.len() - 1));
        } else {
            slot.push(None);
        }
    }
    let used = off.len();
    let (mut status, mut verdict) = (vec![9u8; used], vec![9u8; used]);
    if used > 0 {
        text.push(b' '); // (never an empty buffer; no document reaches it)
        with_ctx(|ctx| {
            ok(unsafe {
                sys::zkp_correct_key_ni_verify_json_batch(ctx, text.as_ptr() as *const std::os::raw::c_char, off.as_ptr(), len.as_ptr(), used as u64, n_bits, n.as_ptr(),
                                                          salt.as_ptr(), salt.len() as u32, status.as_mut_ptr(), verdict.as_mut_ptr(), 0)
            })
        })?;
    }
    Some(
        slot.iter()
            .map(|s| s.and_then(|i| if status[i] != sys::ZKP_DOC_OK { None } else if verdict[i] == sys::ZKP_VERDICT_ACCEPT { Some(Verdict::Accept) } else { Some(Verdict::Reject) }))
            .collect(),
    )
}

/// Single-proof dispatch used by the patched `NiCorrectKeyProof::verify`.
pub fn correct_key_ni_verify_one(proof: &NiCorrectKeyProof, ek: &EncryptionKey, salt: &[u8]) -> Option<Result<(), IncorrectProof>> {
    match correct_key_ni_verify_batch(&[(ek, proof)], salt)?.pop()?? {
        Verdict::Accept => Some(Ok(())),
        Verdict::Reject => Some(Err(IncorrectProof)),
        Verdict::WouldPanic => None,
    }
}

impl NiCorrectKeyProof {
    /// Many keys at once (e.g. the key-generation phase of a threshold-signing ceremony with many parties).
    pub fn verify_batch(items: &[(&EncryptionKey, &NiCorrectKeyProof)], salt: &[u8]) -> Vec<Verdict> {
        let gpu = correct_key_ni_verify_batch(items, salt);
        items
            .iter()
            .enumerate()
            .map(|(k, (ek, proof))| match gpu.as_ref().and_then(|v| v[k]) {
                Some(v) => v,
                None => match std::panic::catch_unwind(std::panic::AssertUnwindSafe(|| proof.verify(ek, salt))) {
                    Ok(Ok(())) => Verdict::Accept,
                    Ok(Err(IncorrectProof)) => Verdict::Reject,
                    Err(_) => Verdict::WouldPanic,
                },
            })
            .collect()
    }
}

// ------------------------------------------------------------------------------------------------ CompositeDLogProof
fn dlog_statement_limbs(statement: &DLogStatement) -> Option<(u32, Vec<u32>, Vec<u32>, Vec<u32>)> {
    let n_bits = width_for(&statement.N)?;
    let kw = (n_bits / 32) as usize;
    let (mut nn, mut g, mut ni) = (vec![0u32; kw], vec![0u32; kw], vec![0u32; kw]);
    if put_limbs(&mut nn, &statement.N) && put_limbs(&mut g, &statement.g) && put_limbs(&mut ni, &statement.ni) {
        Some((n_bits, nn, g, ni))
    } else {
        None
    }
}

/// `CompositeDLogProof::prove` (src/zkproofs/wi_dlog_proof.rs:46-65): x = g^r mod N, e = H(x, g, N, ni), y = r + e s, with the
/// 512-bit nonce sampled here as the reference samples it (:53-54).
pub fn dlog_prove_one(statement: &DLogStatement, secret: &BigInt) -> Option<CompositeDLogProof> {
    let (n_bits, nn, g, ni) = dlog_statement_limbs(statement)?;
    let kw = (n_bits / 32) as usize;
    let yw = (DLOG_Y_BITS / 32) as usize;
    let big_r = BigInt::from(2).pow(512); // K + K_PRIME + SAMPLE_S, :53
    let r = BigInt::sample_below(&big_r); // :54
    let (mut s, mut rr) = (vec![0u32; 8], vec![0u32; yw]);
    if !put_limbs(&mut s, secret) || !put_limbs(&mut rr, &r) {
        return None; // a secret wider than 256 bits: GMP
    }
    let (mut x, mut y) = (vec![0u32; kw], vec![0u32; yw]);
    with_ctx(|ctx| {
        ok(unsafe { sys::zkp_dlog_prove_batch(ctx, n_bits, DLOG_Y_BITS, 1, nn.as_ptr(), g.as_ptr(), ni.as_ptr(), s.as_ptr(), rr.as_ptr(), x.as_mut_ptr(), y.as_mut_ptr(), 0) })
    })?;
    Some(CompositeDLogProof { x: get_limbs(&x), y: get_limbs(&y) })
}

/// `serde_json::from_str` of a `DLogStatement` and a `CompositeDLogProof` document + `verify`, for many pairs of ONE modulus width in one
/// `zkp_dlog_verify_json_batch`: both documents are scanned, converted, range-checked and verified on the GPU.  `bare_form`: the text form
/// curv's `BigInt` has in this build (`sys::ZKP_BIGINT_DEC` / `_HEX` / `_BYTES`).  `None` for a pair: it was not verified here
/// (`ZKP_DOC_INVALID`: serde's error; `ZKP_DOC_HOST_PATH`: a field the layout cannot carry, an even N, g / ni / x >= N; or one of the
/// reference's three assertions would panic) — the caller keeps it on its serde + GMP path, which gives the reference's answer.
pub fn dlog_verify_json_batch(n_bits: u32, bare_form: u32, pairs: &[(&str, &str)]) -> Option<Vec<Option<Result<(), IncorrectProof>>>> {
    if pairs.is_empty() {
        return Some(Vec::new());
    }
    let b = pairs.len();
    let mut text = Vec::<u8>::new();
    let (mut s_off, mut s_len, mut p_off, mut p_len) = (Vec::<u64>::new(), Vec::<u64>::new(), Vec::<u64>::new(), Vec::<u64>::new());
    for (statement, _) in pairs.iter() {
        s_off.push(text.len() as u64);
        s_len.push(statement.len() as u64);
        text.extend_from_slice(statement.as_bytes());
    }
    for (_, proof) in pairs.iter() {
        p_off.push(text.len() as u64);
        p_len.push(proof.len() as u64);
        text.extend_from_slice(proof.as_bytes());
    }
    text.push(b' '); // (never an empty buffer; no document reaches it)
    let (mut status, mut verdict) = (vec![9u8; b], vec![9u8; b]);
    with_ctx(|ctx| {
        ok(unsafe {
            sys::zkp_dlog_verify_json_batch(ctx, text.as_ptr() as *const std::os::raw::c_char, s_off.as_ptr(), s_len.as_ptr(), p_off.as_ptr(), p_len.as_ptr(), b as u64, n_bits,
                                            DLOG_Y_BITS, bare_form, status.as_mut_ptr(), verdict.as_mut_ptr(), 0)
        })
    })?;
    Some(
        (0..b)
            .map(|i| if status[i] != sys::ZKP_DOC_OK { None } else if verdict[i] == sys::ZKP_VERDICT_ACCEPT { Some(Ok(())) } else if verdict[i] == sys::ZKP_VERDICT_REJECT { Some(Err(IncorrectProof)) } else { None })
            .collect(),
    )
}

/// `zkp_json_dlog_statement_batch` on host arrays: N, g, ni `[B][n_bits / 32]`.  Returns the status bytes (`ZKP_DOC_*`).
/// Safety: every output pointer holds `docs.len() * n_bits / 32` words.  (Device-resident outputs: `sys::` with `ZKP_F_DEVICE_PTRS`.)
pub unsafe fn json_dlog_statement_batch(n_bits: u32, bare_form: u32, docs: &[&str], out_n: *mut u32, out_g: *mut u32, out_ni: *mut u32) -> Option<Vec<u8>> {
    let (text, off, len) = pack_docs(docs);
    let mut status = vec![9u8; docs.len()];
    with_ctx(|ctx| ok(sys::zkp_json_dlog_statement_batch(ctx, text.as_ptr() as *const std::os::raw::c_char, off.as_ptr(), len.as_ptr(), n_bits, docs.len() as u64, bare_form, out_n, out_g, out_ni, status.as_mut_ptr(), 0)))?;
    Some(status)
}

/// `zkp_json_dlog_proof_batch` on host arrays: x `[B][n_bits / 32]`, y `[B][768 / 32]`.
pub unsafe fn json_dlog_proof_batch(n_bits: u32, bare_form: u32, docs: &[&str], out_x: *mut u32, out_y: *mut u32) -> Option<Vec<u8>> {
    let (text, off, len) = pack_docs(docs);
    let mut status = vec![9u8; docs.len()];
    with_ctx(|ctx| ok(sys::zkp_json_dlog_proof_batch(ctx, text.as_ptr() as *const std::os::raw::c_char, off.as_ptr(), len.as_ptr(), n_bits, DLOG_Y_BITS, docs.len() as u64, bare_form, out_x, out_y, status.as_mut_ptr(), 0)))?;
    Some(status)
}

fn pack_docs(docs: &[&str]) -> (Vec<u8>, Vec<u64>, Vec<u64>) {
    let (mut text, mut off, mut len) = (Vec::<u8>::new(), Vec::<u64>::new(), Vec::<u64>::new());
    for d in docs.iter() {
        off.push(text.len() as u64);
        len.push(d.len() as u64);
        text.extend_from_slice(d.as_bytes());
    }
    text.push(b' ');
    (text, off, len)
}

/// `serde_json::to_string` of many statements of one width in one `zkp_json_write_dlog_statement_batch` (sizing call, then the writing call).
pub fn json_write_dlog_statement_batch(statements: &[&DLogStatement], bare_form: u32) -> Option<Vec<String>> {
    if statements.is_empty() {
        return Some(Vec::new());
    }
    let n_bits = width_for(&statements[0].N)?;
    let kw = (n_bits / 32) as usize;
    let b = statements.len();
    let (mut nn, mut g, mut ni) = (vec![0u32; b * kw], vec![0u32; b * kw], vec![0u32; b * kw]);
    for (k, s) in statements.iter().enumerate() {
        if !(put_limbs(&mut nn[k * kw..(k + 1) * kw], &s.N) && put_limbs(&mut g[k * kw..(k + 1) * kw], &s.g) && put_limbs(&mut ni[k * kw..(k + 1) * kw], &s.ni)) {
            return None;
        }
    }
    write_docs(b, |ctx, text, cap, off| unsafe { sys::zkp_json_write_dlog_statement_batch(ctx, n_bits, b as u64, nn.as_ptr(), g.as_ptr(), ni.as_ptr(), bare_form, text, cap, off, ptr::null_mut(), 0) })
}

/// `serde_json::to_string` of many proofs under moduli of `n_bits` bits in one `zkp_json_write_dlog_proof_batch`.
pub fn json_write_dlog_proof_batch(n_bits: u32, proofs: &[&CompositeDLogProof], bare_form: u32) -> Option<Vec<String>> {
    if proofs.is_empty() {
        return Some(Vec::new());
    }
    let (kw, yw) = ((n_bits / 32) as usize, (DLOG_Y_BITS / 32) as usize);
    let b = proofs.len();
    let (mut x, mut y) = (vec![0u32; b * kw], vec![0u32; b * yw]);
    for (k, p) in proofs.iter().enumerate() {
        if !(put_limbs(&mut x[k * kw..(k + 1) * kw], &p.x) && put_limbs(&mut y[k * yw..(k + 1) * yw], &p.y)) {
            return None;
        }
    }
    write_docs(b, |ctx, text, cap, off| unsafe { sys::zkp_json_write_dlog_proof_batch(ctx, n_bits, DLOG_Y_BITS, b as u64, x.as_ptr(), y.as_ptr(), bare_form, text, cap, off, ptr::null_mut(), 0) })
}

/// sizing call, one allocation, writing call; documents cut at the offsets
fn write_docs<F: Fn(*mut sys::zkp_ctx, *mut std::os::raw::c_char, u64, *mut u64) -> i32>(b: usize, call: F) -> Option<Vec<String>> {
    let mut off = vec![0u64; b + 1];
    with_ctx(|ctx| ok(call(ctx, ptr::null_mut(), 0, off.as_mut_ptr())))?;
    let mut text = vec![0u8; off[b] as usize + 1];
    let total = off[b];
    with_ctx(|ctx| ok(call(ctx, text.as_mut_ptr() as *mut std::os::raw::c_char, total, off.as_mut_ptr())))?;
    Some((0..b).map(|k| String::from_utf8_lossy(&text[off[k] as usize..off[k + 1] as usize]).into_owned()).collect())
}

/// `CompositeDLogProof::verify` (wi_dlog_proof.rs:67-91).  `None` also when the reference's pre-checks would panic (:69,72,73):
/// the GMP path then raises that panic.
pub fn dlog_verify_one(proof: &CompositeDLogProof, statement: &DLogStatement) -> Option<Result<(), IncorrectProof>> {
    let (n_bits, nn, g, ni) = dlog_statement_limbs(statement)?;
    let kw = (n_bits / 32) as usize;
    let yw = (DLOG_Y_BITS / 32) as usize;
    let (mut x, mut y) = (vec![0u32; kw], vec![0u32; yw]);
    if !put_limbs(&mut x, &proof.x) || !put_limbs(&mut y, &proof.y) {
        return None;
    }
    let mut verdict = [9u8; 1];
    with_ctx(|ctx| {
        ok(unsafe { sys::zkp_dlog_verify_batch(ctx, n_bits, DLOG_Y_BITS, 1, nn.as_ptr(), g.as_ptr(), ni.as_ptr(), x.as_ptr(), y.as_ptr(), verdict.as_mut_ptr(), 0) })
    })?;
    match verdict[0] {
        sys::ZKP_VERDICT_ACCEPT => Some(Ok(())),
        sys::ZKP_VERDICT_REJECT => Some(Err(IncorrectProof)),
        _ => None,
    }
}
