{-# LANGUAGE ForeignFunctionInterface #-}
-- | Device back end of "Data.Text.AhoCorasick.Splitter" (reference: src/Data/Text/AhoCorasick/Splitter.hs):
-- 'split' (:84-85) and 'splitIgnoreCase' (:96-97) for batches of haystacks.
--
-- A 'DeviceSplitter' is a reference 'Splitter.Splitter' plus its one-needle automaton in HBM and the separator's
-- length in bytes (:105) and in code points (:117).  The scan and the fold 'stepAccum' / 'finalizeAccum' (:141-170)
-- both run on the device; what comes back is a (start, length) pair per fragment, and the fragments are slices of
-- the haystacks ('Utf8.unsafeSliceUtf8', as the reference builds them): no byte of text is copied.
module Data.Text.AhoCorasick.Splitter.Device
  ( DeviceSplitter
  , toDevice
  , splitter
  , split
  , splitIgnoreCase
  ) where

import Control.Exception (finally)
import Control.Monad (when)
import Data.List.NonEmpty (NonEmpty)
import Data.Word (Word32, Word64)
import Foreign
import Foreign.C.Types

import qualified Data.List.NonEmpty as NonEmpty
import qualified Data.Text as Text

import Data.Text.AhoCorasick.Automaton (CaseSensitivity (..), CodeUnitIndex (..))
import Data.Text.Utf8 (Text)

import qualified Data.Text.AhoCorasick.Automaton.Device as Dev
import qualified Data.Text.AhoCorasick.Splitter as Splitter
import qualified Data.Text.Utf8 as Utf8

data AmSplitter
data AmFragments

foreign import ccall unsafe "am_splitter_create"
  c_am_splitter_create :: Ptr Dev.AmAutomaton -> Word32 -> Word32 -> Ptr (Ptr AmSplitter) -> IO CInt
foreign import ccall unsafe "&am_splitter_destroy"
  p_am_splitter_destroy :: FunPtr (Ptr AmSplitter -> IO ())
foreign import ccall safe "am_split"
  c_am_split :: Ptr AmSplitter -> CInt -> Ptr Dev.AmSlice -> CSize -> Ptr (Ptr AmFragments) -> IO CInt
foreign import ccall unsafe "am_fragments_size"
  c_am_fragments_size :: Ptr AmFragments -> IO Word64
foreign import ccall safe "am_fragments_offsets"
  c_am_fragments_offsets :: Ptr AmFragments -> IO (Ptr Word64)
foreign import ccall safe "am_fragments_data"
  c_am_fragments_data :: Ptr AmFragments -> IO (Ptr Word64)
foreign import ccall unsafe "am_fragments_free"
  c_am_fragments_free :: Ptr AmFragments -> IO ()

data DeviceSplitter = DeviceSplitter
  { dsSplitter :: !Splitter.Splitter
  , dsMachine  :: !(Dev.DeviceMachine ())
  , dsHandle   :: !(ForeignPtr AmSplitter)
  }

-- | The reference splitter inside (for 'Splitter.separator', 'Splitter.automaton').
splitter :: DeviceSplitter -> Splitter.Splitter
splitter = dsSplitter

toDevice :: Splitter.Splitter -> IO DeviceSplitter
toDevice s = do
  dm <- Dev.toDevice (Splitter.automaton s)
  let sep      = Splitter.separator s
      CodeUnitIndex sepBytes = Utf8.lengthUtf8 sep
      sepCps   = Text.length sep
  h <- withForeignPtr (Dev.dmHandle dm) $ \pa -> alloca $ \out -> do
    c_am_splitter_create pa (fromIntegral sepBytes) (fromIntegral sepCps) out >>= Dev.checkRc
    peek out >>= newForeignPtr p_am_splitter_destroy
  pure (DeviceSplitter s dm h)

-- | 'Splitter.split' (Splitter.hs:84-85) for a batch.
split :: DeviceSplitter -> [Text] -> IO [NonEmpty Text]
split = splitWithCase CaseSensitive

-- | 'Splitter.splitIgnoreCase' (Splitter.hs:96-97) for a batch; the splitter must have been built with a lower-case separator (:92-93).
splitIgnoreCase :: DeviceSplitter -> [Text] -> IO [NonEmpty Text]
splitIgnoreCase = splitWithCase IgnoreCase

splitWithCase :: CaseSensitivity -> DeviceSplitter -> [Text] -> IO [NonEmpty Text]
splitWithCase cs ds texts =
  Dev.withPinnedTexts texts $ \pSlices n ->
    withForeignPtr (dsHandle ds) $ \ph -> withForeignPtr (Dev.dmHandle (dsMachine ds)) $ \_ -> alloca $ \out -> do
      c_am_split ph (Dev.caseFlag cs) pSlices (fromIntegral n) out >>= Dev.checkRc
      frs <- peek out
      -- the result is freed on every path, also when a copy to the host fails
      (offs, flat) <- (`finally` c_am_fragments_free frs) $ do
        total <- c_am_fragments_size frs
        pOff  <- c_am_fragments_offsets frs
        pData <- c_am_fragments_data frs
        when (pOff == nullPtr || pData == nullPtr) $ Dev.checkRc (-3)
        (,) <$> peekArray (n + 1) pOff <*> peekArray (2 * fromIntegral total) pData
      let pairs (a : b : rest) = (a, b) : pairs rest
          pairs _              = []
          slice hay (start, len) = Utf8.unsafeSliceUtf8 (CodeUnitIndex (fromIntegral start)) (CodeUnitIndex (fromIntegral len)) hay
          counts = zipWith (\o0 o1 -> fromIntegral (o1 - o0)) offs (drop 1 offs) :: [Int]
          -- one pass over the fragments: every haystack takes its own from the front of what is left
          go _ [] = []
          go rest ((hay, k) : more) = let (mine, rest') = splitAt k rest in NonEmpty.fromList (map (slice hay) mine) : go rest' more
      -- every haystack has at least one fragment (finalizeAccum, Splitter.hs:141-147)
      pure (go (pairs flat) (zip texts counts))
