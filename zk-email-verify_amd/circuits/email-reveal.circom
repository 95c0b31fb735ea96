pragma circom 2.1.6;

include "@zk-email/circuits/email-verifier.circom";
include "@zk-email/circuits/helpers/reveal-substring.circom";
include "@zk-email/circuits/helpers/email-nullifier.circom";
include "@zk-email/circuits/utils/bytes.circom";

/// @title EmailReveal
/// @notice An application circuit over EmailVerifier: proves that a DKIM-signed email exists AND makes a substring of its
///         header (or body) public, packed 31 bytes per signal, together with the signer's key hash and, optionally, a
///         nullifier of the email.  This is the circuit ZKWG_MAIN_EMAIL_REVEAL computes witnesses for; compile this file
///         (with `@zk-email/circuits` and `circomlib` on the include path) to get the matching proving key.
/// @param maxHeadersLength, maxBodyLength, n, k, ignoreBodyHashCheck  as in EmailVerifier (masking and soft-line-break
///         removal are off)
/// @param revealFromBody          0: the substring is taken from emailHeader, 1: from emailBody
/// @param maxSubstringLength      maximum number of revealed bytes
/// @param shouldCheckUniqueness   1: the revealed bytes must occur exactly once in the source
/// @param withNullifier           1: output emailNullifier = Poseidon(Poseidon(signature))
/// @input  EmailVerifier's inputs, then substringStartIndex and substringLength
/// @output pubkeyHash, (withNullifier) emailNullifier, revealed[computeIntChunkLength(maxSubstringLength)]
template EmailReveal(maxHeadersLength, maxBodyLength, n, k, ignoreBodyHashCheck, revealFromBody, maxSubstringLength, shouldCheckUniqueness, withNullifier) {
    assert(revealFromBody == 0 || revealFromBody == 1);
    assert(shouldCheckUniqueness == 0 || shouldCheckUniqueness == 1);
    assert(withNullifier == 0 || withNullifier == 1);
    // the body is only bound to the signature when its hash is checked
    assert(revealFromBody == 0 || ignoreBodyHashCheck != 1);

    var maxInts = computeIntChunkLength(maxSubstringLength);

    signal input emailHeader[maxHeadersLength];
    signal input emailHeaderLength;
    signal input pubkey[k];
    signal input signature[k];

    signal output pubkeyHash;
    if (withNullifier == 1) {
        // (declared and assigned in one block: a signal is visible only inside the block that declares it)
        signal output emailNullifier;
        emailNullifier <== EmailNullifier(n, k)(signature);
    }
    signal output revealed[maxInts];

    component ev = EmailVerifier(maxHeadersLength, maxBodyLength, n, k, ignoreBodyHashCheck, 0, 0, 0);
    ev.emailHeader <== emailHeader;
    ev.emailHeaderLength <== emailHeaderLength;
    ev.pubkey <== pubkey;
    ev.signature <== signature;

    var maxLength = maxHeadersLength;
    if (revealFromBody == 1) {
        maxLength = maxBodyLength;
    }
    component rs = RevealSubstring(maxLength, maxSubstringLength, shouldCheckUniqueness);

    if (ignoreBodyHashCheck != 1) {
        signal input bodyHashIndex;
        signal input precomputedSHA[32];
        signal input emailBody[maxBodyLength];
        signal input emailBodyLength;

        ev.bodyHashIndex <== bodyHashIndex;
        ev.precomputedSHA <== precomputedSHA;
        ev.emailBody <== emailBody;
        ev.emailBodyLength <== emailBodyLength;

        if (revealFromBody == 1) {
            rs.in <== emailBody;
        }
    }
    if (revealFromBody == 0) {
        rs.in <== emailHeader;
    }
    pubkeyHash <== ev.pubkeyHash;

    signal input substringStartIndex;
    signal input substringLength;

    rs.substringStartIndex <== substringStartIndex;
    rs.substringLength <== substringLength;

    revealed <== PackBytes(maxSubstringLength)(rs.substring);
}

// The outputs are the statement, so a main has no public inputs, e.g. a 32-byte unique substring of a 1024-byte header:
//   component main = EmailReveal(1024, 1536, 121, 17, 0, 0, 32, 1, 1);
